// Host-callable launchers of the HIP kernels (kernels_records.hip, kernels_build.hip, kernels_refit.hip, kernels_render.hip, kernels_path.hip, kernels_post.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "device/trace_split.h"
#include "device/types.h"
#include "glaze_abi.h"
#include "device_buffer.h"
#include "reproject.h"

namespace glz {

// ---- scene build --------------------------------------------------------------------------------
hipError_t launch_derivatives(hipStream_t st, const float4* vertices, const uint32_t* indices, uint32_t n_tris, float4* out);

struct HierarchyInputs {
  const float4* vertices;
  const uint32_t* indices;
  const RTInstance* instances;
  const uint32_t* inst_base;   // exclusive prefix sum of triangles per instance (n_instances entries)
  uint32_t n_instances;
  const TransformPair* transforms;
  const RTMaterial* materials;
  uint32_t n_world;
  int builder;                 // kBvhBuilder*
  float pair_area_ratio;       // two triangles share a leaf when area(joint box) <= ratio * (area(a) + area(b)); 0 = never (k_pair_triangles)
  // Hierarchy over GIVEN boxes instead of triangles (the instance level of a two-level structure): n_world boxes, box i becomes a
  // one-"triangle" leaf whose BvhTri::world_id is i; vertices / indices / instances are not read.  Device pointers; null = triangles.
  const float4* given_lo = nullptr;
  const float4* given_hi = nullptr;
  // The flattened world build: also emit the 64-byte per-leaf records (BvhQuad) and make leaf links ~leaf number instead of
  // ~first triangle slot (the record names the slot).  Pairs are only formed in the two vertex orders a quad record can hold.
  bool emit_quads = false;
  // ... and the same hierarchy collapsed eight wide (types.h BvhNode8; needs emit_quads): HierarchyOutputs::nodes8
  bool emit_wide8 = false;
};
constexpr int kBvhBuilderLbvh = 0, kBvhBuilderPloc = 1, kBvhBuilderSah = 2, kBvhBuilderAuto = 3, kBvhBuilderSahHost = 4;   // = GLZ_BVH_LBVH / _PLOC / _SAH / _AUTO / _SAH_HOST
// host side of the SAH builder (bvh_sah.cpp): binary hierarchy over n leaf boxes -> children / parent arrays
void build_sah_host(uint32_t n, const float4* lo, const float4* hi, int2* children, int* parent);
// nodes / nodes8 / quads are allocated by build_hierarchy and owned by this struct: what the caller wants to keep it moves out, the rest is
// freed with the struct -- also after a failed build, whatever it got to.  Their .count is the number of entries.
struct HierarchyOutputs {
  DeviceBuffer<BvhNode4> nodes;    // empty for n_world = 0
  DeviceBuffer<BvhNode8> nodes8;   // emit_wide8, else empty; a scene of one leaf has none
  uint32_t depth8;
  BvhGrid grid;     // quantisation grid of the node boxes
  BvhTri* tris;     // n_world + 1 entries (the tracer reads one past a leaf's first triangle), preallocated by the caller; leaf order, a leaf's triangles adjacent
  DeviceBuffer<BvhQuad> quads;     // emit_quads: one record per leaf, else empty
  uint32_t depth;   // number of 4-wide nodes above the deepest leaf (the traversal stack holds at most 3 * depth + 1 entries)
  float sah;
  float bounds_lo[3], bounds_hi[3];
};
hipError_t build_hierarchy(hipStream_t st, const HierarchyInputs& in, HierarchyOutputs& out);
// top-of-tree table for LDS staging (types.h kBvhTopNodes): `top` receives kBvhTopNodes nodes
hipError_t launch_top_table(hipStream_t st, const BvhNode4* nodes, uint32_t n_nodes, BvhNode4* top);
// 128-byte per-leaf shading records (see k_shade_records); xf_identity[t] != 0 marks an exact identity transform
hipError_t launch_shade_records(hipStream_t st, uint32_t n, const BvhTri* tris, const RTInstance* instances, const uint32_t* indices,
                                const float4* vertices, const float4* derivatives, const uint32_t* xf_identity, float4* out);
// Instance boxes of a two-level top level (kernels_tlas.hip, Scene::update_transforms): item j takes the world positions of
// points[first .. first + count) under transform `transform`; an instance's items are item_first[i] .. item_first[i + 1] (at least one),
// all naming the same transform and mesh.  partial: 6 doubles per item (scratch).
struct InstanceBoxItem {
  uint32_t transform, mesh, first, count;
};
hipError_t launch_instance_boxes(hipStream_t st, uint32_t n_items, const InstanceBoxItem* items, const float4* points, const TransformPair* xf,
                                 double* partial, uint32_t n_instances, const uint32_t* item_first, const float4* mesh_lo, const float4* mesh_hi,
                                 float4* box_lo, float4* box_hi);
// DeviceScene::alpha_recs for `n` triangle slots (flattened scenes with an opacity map)
hipError_t launch_alpha_records(hipStream_t st, uint32_t n, const float4* shade_tris, const RTMaterial* materials, const TexDesc* tex_desc, float4* out);

// ---- refit (kernels_refit.hip, Accel::update_geometry): new vertices under a hierarchy that keeps its topology ----
// The leaf records `quads` (each names its instance, first primitive and first triangle slot) written again from the vertices, with
// their triangles in `tris` and their float boxes in leaf_lo / leaf_hi, all by the build's rules.
hipError_t launch_refit_leaves(hipStream_t st, const float4* vertices, const uint32_t* indices, const RTInstance* instances, const TransformPair* transforms,
                               uint32_t n_leaves, BvhQuad* quads, BvhTri* tris, float4* leaf_lo, float4* leaf_hi);
// One width of a structure's wide nodes with what the level launches need (the refit plan): the nodes grouped by height above the
// leaves -- order[level_first[h] .. level_first[h + 1]) are those of height h -- and a float box per node and per leaf.
struct RefitNodes {
  int width;        // 4 (BvhNode4) or 8 (BvhNode8)
  void* nodes;
  uint32_t n_nodes;
  const uint32_t* order;   // device
  const std::vector<uint32_t>& level_first;
  const float4 *leaf_lo, *leaf_hi;
  float4 *node_lo, *node_hi;
};
// node boxes from the leaf boxes up, one launch per level; then the grid from a root box; then every child box on that grid again
// (write = false leaves the nodes alone) and, with `area`, the sum of the child boxes' surface areas added to *area
hipError_t launch_refit_fit(hipStream_t st, const RefitNodes& n);
hipError_t launch_refit_grid(hipStream_t st, const float4* root_lo, const float4* root_hi, BvhGrid* grid);
hipError_t launch_refit_quantise(hipStream_t st, const RefitNodes& n, const BvhGrid* grid, bool write, float* area);

// Traversal stack entries each lane keeps in LDS (a near-first 4-wide traversal holds at most three entries per
// level of the tree; what does not fit spills to a per-lane HBM area).
constexpr int kTraversalLdsStack = 17;   // 17 levels + the staged top of the tree = 25 920 bytes per block: six blocks per CU (LDS is granted in 1 280-byte granules: 18 levels + the table would take 22 granules and leave room for five)
constexpr int kPersistentBlocksPerCuMax = 8;   // the most blocks per CU a persistent tracer's grid is given (launch_geometry.h resident_blocks)

// The tracers fetch nodes, leaf records, instance records and spilt stack words at a wave-uniform base plus a 32-bit BYTE offset per
// lane (device/trace_wave.h record_at, StackT), so each of these must be shorter than 2^32 bytes: 4-wide nodes and leaf records of 64
// bytes, 8-wide nodes of 128, instance records of 192, and the spill area of the largest persistent grid, overflow_depth words a lane.
// Null when all of them fit, else the message that says which does not.  (The largest scene built so far, 21 M triangles, is a tenth of it.)
struct TraversalSizes {
  uint64_t n_nodes, n_nodes8, n_leaves, n_instances, grid_lanes, overflow_depth;
};
const char* traversal_offsets_exceeded(const TraversalSizes& sizes);   // accel.cpp

// ---- rendering ------------------------------------------------------------------------------------
// Per-pixel wavefront state, indexed by the LOCAL pixel id `lid` (tile-major, one wave = one 8x8 block):
//   lid = ((local_tile * 64 + sub_block) * 64 + lane)
struct PathState {
  float4* ray_o;     // origin.xyz, bounce number        (PTLastVertex.hit, raytrace_structures.rs:89-95)
  float4* ray_d;     // direction.xyz, last-bounce-specular flag (PTLastVertex.wi)
  float4* imp[4];    // importance spectrum, 4 x vec4    (PTLastVertex.importance)
  float4* hit;       // t, u, v, leaf index (bits)       closest-hit record of the current launch
  float* cone;       // ray-cone width at the ray origin (texture LOD, FrameData::lod_mode; untouched when it is off)
  uint32_t* hit_inst;// RTInstance of the closest hit (two-level scenes only: a flattened triangle record names its instance)
  // shadow-ray queue, compacted by k_shade (entry q, not pixel lid):
  float4* sh_o;      //   origin.xyz, tmax
  float4* sh_d;      //   direction.xyz, owning pixel lid (bits)
  float4* contrib;   //   rgb radiance to add if unoccluded, flags (bits)
  uint32_t* queue_count;
  float4* cumulative;// accumulate_image (xyz = sum rgb, w = launches; between two resolves w < 0 marks the launch of the last update: device/path_state.h)
  float4* result;    // result_image (out32), written by k_finalize
  uint32_t* overflow;// traversal stack spill, `overflow_depth` words per lane slot of the k_trace grid
  uint32_t overflow_depth;
  uint32_t* path_cost;// k_path: [0..7] two accumulators {sum of per-launch ticks (u64), groups (u32), pad}, then one word per 64-pixel group: its ticks per launch in the last batch
};

struct TileMap {
  uint32_t width, height;
  uint32_t tiles_x, tiles_y;
  uint32_t rank, world;      // this renderer owns global tiles t with t % world == rank
  uint32_t n_local_tiles;
  uint32_t n_local_pixels;   // n_local_tiles * 4096
};

struct CameraConsts {
  float camera2world[16];
  float screen2camera[16];
};

struct TraceCounters {
  unsigned long long closest_rays, shadow_rays, closest_nodes, closest_tris, shadow_nodes, shadow_tris, hits, fresh;
  unsigned long long phase[12];   // {node_iters, node_lanes, leaf_iters, leaf_lanes, refill_iters, refill_lanes} x {closest, shadow}
  // DeviceScene::tex_counter of k_shade / of k_trace (alpha tests): {fetches, texel bytes, light samples other than sky, sky-light samples}
  unsigned long long shade_tex[4], trace_tex[4];
};

struct LaunchArgs {
  DeviceScene scene;
  PathState st;
  TileMap map;
  FrameData frame;
  CameraConsts cam;
  TraceCounters* counters;   // nullptr unless counting is enabled
  // k_trace phases of this call: closest-hit rays of the current launch and / or the shadow rays the PREVIOUS launch's
  // k_shade queued (they only gate an accumulation, so nothing of the current launch depends on them)
  uint32_t do_closest, do_shadow;
  uint32_t shade_set;        // which of the two shadow-queue counter sets this launch's k_shade fills (the other one is drained)
  float shadow_mark;         // FrameData::update_mark of the launch that queued the shadow rays
  TraceSplitTuning split;    // k_trace: how the waves divide the two kinds of group (device/trace_split.h; the defaults of device/tuning.h unless GLAZE_TRACE_SPLIT says otherwise)
};
// The launches one k_path call runs (kernels_path.hip): what differs between launches, by value in the kernel arguments (12 bytes a
// launch next to the 880 of LaunchArgs: 192 launches stay inside the 4 KB the arguments may take).  Long batches matter: the kernel
// ends when its slowest wave does, and a wave's time per launch scatters by ~20 % -- over 16 launches the slowest of 4 096 waves is
// 27 % above the mean, over 192 launches 8 %.
constexpr uint32_t kPathMaxLaunches = 192;
struct PathBatch {
  uint32_t n;                              // launches in this call
  uint32_t tables_in_lds;                  // filled by launch_path
  uint32_t parity;                         // which of the two cost accumulators this batch adds to (it reads the other one)
  uint32_t seed[kPathMaxLaunches];         // FrameData::seed of each launch (the rest of FrameData is LaunchArgs::frame)
  float offset[kPathMaxLaunches + 1][2];   // FrameData::pixel_offset; entry n: of the launch after the batch (FrameData::next_pixel_offset)
  uint32_t base_ordinal;                   // accumulating launches since the reset before this batch: launch L of it is number base_ordinal + L + 1 (FrameData::update_mark)
};
constexpr uint32_t kTraceBlock = 256;          // threads per block of the render kernels (4 waves)
constexpr uint32_t kQueueSetWords = 8 * 32;   // 8 shard counters, 128 bytes apart
// PathState::queue_count: the two counter sets, then per set the head of its shadow-group pool (device/trace_split.h), each on a 128-byte line of its own
constexpr uint32_t kPoolHeadStride = 32;
constexpr uint32_t kQueueCountWords = 2 * kQueueSetWords + 2 * kPoolHeadStride;
constexpr uint32_t pool_head_word(uint32_t set) { return 2 * kQueueSetWords + set * kPoolHeadStride; }

// persistent grid of k_trace / k_trace_tl / (wide8) k_trace8 (device must be current); wide8: the walk over the 8-wide nodes, flattened scenes without work counters
uint32_t trace_grid_blocks(uint32_t n_local_pixels, bool counting, bool two_level, bool wide8 = false);
hipError_t launch_trace(hipStream_t st, const LaunchArgs& a, uint32_t blocks, bool wide8 = false);
hipError_t launch_shade(hipStream_t st, const LaunchArgs& a);
// the per-wave launch loop of a small tile share: `batch.n` launches for every pixel in ONE kernel (a.frame holds what the launches
// share; flattened scenes, no work counters); blocks from path_grid_blocks (device must be current)
uint32_t path_grid_blocks(uint32_t n_local_pixels, const DeviceScene& scene);
uint32_t path_resident_blocks(const DeviceScene& scene);   // blocks of k_path the chip holds at once
hipError_t launch_path(hipStream_t st, const LaunchArgs& a, const PathBatch& batch, uint32_t blocks);
// The resolve (Renderer::settle): for every pixel of the chain that updated since the last one (cumulative.w < 0) result = xyz * exposure / -w,
// then cumulative.w = launches for every active pixel: what update_count / update_result would have left had they run in every launch
hipError_t launch_finalize(hipStream_t st, const TileMap& map, float4* cumulative, float4* result, float exposure, float launches);
// scatter the tile-major cumulative / result images into full-frame row-major RGBA32F buffers
hipError_t launch_export(hipStream_t st, const TileMap& map, const float4* tiled, float4* frame, bool zero_first);
// chain `chain` of `n_chains` -> the rank's packed tile order (local tile j = jl * n_chains + chain), see Renderer::export_packed
hipError_t launch_pack_tiles(hipStream_t st, uint32_t n_chain_pixels, uint32_t n_chains, uint32_t chain, const float4* tiled, float4* packed);
// result (out32) -> RGBA8 sRGB, full-frame row-major (the blit of raytracer.rs:576-584)
// thresholds: 256 floats, [k] = smallest linear value that encodes to k (host::srgb8_thresholds); [0] = 0
hipError_t launch_tonemap(hipStream_t st, uint32_t n_pixels, const float4* result_frame, const float* thresholds, uchar4* out);

// ---- post (kernels_post.hip): first-hit feature buffers and the a-trous denoiser ------------------------
// The first-hit pass: one centre ray per pixel of the FULL frame (a.map: rank 0, world 1; a.frame: scene_size and camera_persp; a.cam;
// a.st.overflow / overflow_depth: one spill slot per lane of `blocks` blocks, from first_hit_grid_blocks with the device current).
// `hit` (t, u, v, leaf bits) and `inst` are private row-major buffers of width * height entries; the attribute kernel turns them into
// aov0 = (normal.xyz, depth) and aov1 = (albedo.rgb, instance bits), row-major.
uint32_t first_hit_grid_blocks(uint32_t n_rays);
hipError_t launch_first_hit(hipStream_t st, const LaunchArgs& a, uint32_t blocks, float4* hit, uint32_t* inst);
hipError_t launch_first_hit_attributes(hipStream_t st, const LaunchArgs& a, const float4* hit, const uint32_t* inst, float4* aov0, float4* aov1);
// Through-specular guides (GLZ_GUIDE_THROUGH_SPECULAR), after launch_first_hit on the same stream and with the same `a`: vertex 0 of every
// pixel, then per bounce k = 1 .. max_bounces the closest hits of list k and vertex k of its rays.  List k (segment k of the chains that have
// one) is compacted: o = (origin, depth so far), d = (direction, pixel bits), in buffers [k & 1] of width * height entries each, its length
// in count[k]; `hit` / `inst` are reused, indexed by list slot.  Nothing is read back: a kernel whose list is empty returns at once.
// blocks: guide_grid_blocks (the device must be current).  last_list: stop once list `last_list` has been written (the planes are then
// those of the vertices so far); GLZ_GUIDE_MAX_BOUNCES + 1 or more runs the whole chain.
constexpr uint32_t kGuideCountWords = GLZ_GUIDE_MAX_BOUNCES + 2;
struct GuideLists {
  float4* o[2];
  float4* d[2];
  uint32_t* count;   // kGuideCountWords words
};
uint32_t guide_grid_blocks(uint32_t n_rays, uint32_t first_hit_blocks);
hipError_t launch_guide_chain(hipStream_t st, const LaunchArgs& a, uint32_t blocks, uint32_t max_bounces, uint32_t last_list, float4* hit, uint32_t* inst,
                              const GuideLists& lists, float4* aov0, float4* aov1);
// list `list` (1 .. GLZ_GUIDE_MAX_BOUNCES) back to its pixels: 3 floats each, row-major, alive = 1; pixels without a ray in it are left as they are
hipError_t launch_guide_scatter(hipStream_t st, uint32_t blocks, const GuideLists& lists, uint32_t list, uint32_t n_pixels, float* origins3, float* dirs3,
                                uint8_t* alive);
// camera_ray() of every pixel at one sub-pixel offset, row-major, 3 floats each
hipError_t launch_camera_rays(hipStream_t st, const LaunchArgs& a, float off_x, float off_y, float* origins3, float* dirs3);
// The filter of glz_denoise_params on row-major device frames: demodulation, `iterations` a-trous passes (one launch each, ping-pong),
// re-modulation in the last pass's store.  ping, pong and out are three different frames of w * h pixels; out may not alias an input.
// marks (timing, may be null): 2 + iterations events recorded before the demodulation, after it and after every pass.
// despeckle (may be null = exactly the launches above): the firefly rejection of glz_despeckle_params between the demodulation and the first
// pass, ping -> pong, the passes then start from pong.  despeckle_marks (may be null): two events recorded around k_despeckle alone.
hipError_t launch_denoise(hipStream_t st, uint32_t w, uint32_t h, const glz_denoise_params& params, const float4* result, const float4* aov0,
                          const float4* aov1, float4* ping, float4* pong, float4* out, hipEvent_t* marks = nullptr,
                          const glz_despeckle_params* despeckle = nullptr, hipEvent_t* despeckle_marks = nullptr);
// The rejection alone: demodulation into ping, then out = i_0' * max(albedo, eps_albedo) in k_despeckle's store.  No a-trous pass.
hipError_t launch_despeckle(hipStream_t st, uint32_t w, uint32_t h, const glz_despeckle_params& params, float eps_albedo, const float4* result,
                            const float4* aov0, const float4* aov1, float4* ping, float4* out, hipEvent_t* despeckle_marks = nullptr);
// Motion and reprojection (reproject.h).  launch_motion: after launch_first_hit on the same stream and with the same `a`, BEFORE the
// attribute kernel or the guide chain (the chain reuses `hit` / `inst`); prev_o2w: one column-major 4x4 per transform of the scene, 64 B
// apart, or null = the scene's own; motion: width * height float4; prev_vertices: null (k_motion), or the previous contents of the scene's
// vertices [first_vertex, first_vertex + n_vertices), two float4 each as the scene stores them, the range inside the scene's vertex count
// (k_motion_deform: the caller has checked the range, the kernel indexes by it).  launch_reproject: all frames are device memory, w * h
// float4 each, out may not alias an input; marks (may be null): two events around the kernel.
hipError_t launch_motion(hipStream_t st, const LaunchArgs& a, const float4* hit, const uint32_t* inst, const float4* prev_o2w, const post::ProjectConstants& prev,
                         float4* motion, const float4* prev_vertices = nullptr, uint32_t first_vertex = 0, uint32_t n_vertices = 0);
hipError_t launch_reproject(hipStream_t st, uint32_t w, uint32_t h, const glz_reproject_params& params, const float4* motion, const float4* prev_color,
                            const float4* prev_aov0, const float4* prev_aov1, float4* out, hipEvent_t* marks = nullptr);
hipError_t launch_project_points(hipStream_t st, const post::ProjectConstants& C, uint32_t w, uint32_t h, const float* points3, uint32_t n, float* out3);

// ---- vertex deformers: morph targets, then skinning (kernels_deform.hip; morph.h and skin.h hold the rules and the layouts) ----
// What the skin step reads.  bind: two float4 a vertex; joints: four uint16 a vertex as one uint2; weights: one float4 a vertex; bones:
// post::bone_rows(blend) float4 a bone (post::pack_bone: three rows; post::pack_bone_dq: two), every joint below n_bones (the caller has
// checked: the kernel indexes by them).  The bone table is staged in LDS when n_bones <= kSkinLdsBones, else read from memory.
struct SkinArgs {
  const float4* bind;
  const uint2* joints;
  const float4* weights;
  uint32_t n;
  const float4* bones;
  uint32_t n_bones;
  int blend;   // GLZ_SKIN_*: the linear rule (k_skin) or the dual-quaternion rule (k_skin_dq)
};
constexpr uint32_t kSkinLdsBones = 256;   // 12 KB of a block's LDS under the linear rule, 8 KB under the dual-quaternion rule
// What the morph step reads: post::MorphLayout on the device, and the base of its n vertices (two float4 a vertex).  Every row's count is
// at most its slice's width and every entry's target below n_targets (pack_morph made them so: the kernel indexes by them).
struct MorphArgs {
  const float4* base;
  const uint32_t* counts;
  const uint2* slices;
  const float4* entries;
  uint32_t n;
  const float* weights;   // n_targets of them, staged in LDS when n_targets <= kMorphLdsTargets, else read from memory
  uint32_t n_targets;
};
constexpr uint32_t kMorphLdsTargets = 1024;   // 4 KB of a block's LDS
// out[2 * i], out[2 * i + 1] = vertex i, i < n, of the morph's base under the morph rule (skin null: k_morph), of the skin's bind pose under
// its skinning rule (morph null: k_skin, k_skin_dq), or of the base -- the skin's bind pose -- under the morph rule and then the skinning
// rule, one store (k_morph_skin, k_morph_skin_dq; n is the morph's).  out: n vertices of device memory that overlap no input.  Nothing is
// launched for no vertices; both null is hipErrorInvalidValue.
hipError_t launch_deform(hipStream_t st, const MorphArgs* morph, const SkinArgs* skin, float4* out);

// ---- skeletons and clips: the bone and weight tables the deformers read, made from keyframes (kernels_clip.hip; clip.h holds the rule) ----
// One clip with its skeleton, as it lies on the device from add_clip on.  Keys: key after key, bone after bone within a key (translations
// and scales 3 floats a bone, rotations 4; scales null: every scale is 1), morph_weights n_targets a key (null: no weight track).
// Skeleton: parents (-1, or below the bone's own index), the level table (clip_levels: level l is level_bones[level_offsets[l] ..
// level_offsets[l + 1]), every entry below n_bones), inverse_bind as three rows a bone with root's three rows behind the last bone's.
// What the kernel writes: world (three rows a bone, scratch), bones (the skin's table: at least 3 * n_bones float4) and weights (n_targets).
struct ClipArgs {
  const float* translations;
  const float* rotations;
  const float* scales;
  const float* morph_weights;
  const int32_t* parents;
  const uint32_t* level_bones;
  const uint32_t* level_offsets;
  const float4* inverse_bind;
  float4* world;
  float4* bones;
  float* weights;
  uint32_t n_bones, n_levels, n_targets;
};
// One play of a call: which clip, the two keys (both below the clip's key count) and the second's weight, and the skin's blend mode now
struct ClipPlay {
  const ClipArgs* clip;
  uint32_t k0, k1;
  float u;
  int blend;   // GLZ_SKIN_*: which layout the bone table gets
};
// One block a play: clip.bones and clip.weights of every play, by THE CLIP RULE.  plays: n_plays of them on the device; no two name
// clips that share a world or bone table.  Nothing is launched for no plays.
hipError_t launch_clip_bones(hipStream_t st, const ClipPlay* plays, uint32_t n_plays);

// ---- vertex normals from deformed positions (kernels_normals.hip; normals.h holds the rule and the layout) ----
// What a normal set's kernels read: post::NormalLayout on the device.  Every face's three indices are below the scene's vertex count,
// every row entry below n_faces and every row's count at most its slice's width (pack_normals made them so: the kernels index by them).
struct NormalArgs {
  const uint32_t* faces;    // 3 a face: indices into the scene's vertex buffer
  uint32_t n_faces;
  const uint32_t* counts;   // one a vertex of the set
  const uint2* slices;
  const uint32_t* rows;
  uint32_t n;               // the set's vertices
};
// face_vectors[f] = the face vector of face f from `vertices`, the scene's WHOLE vertex buffer (two float4 a vertex), f < n_faces
hipError_t launch_face_vectors(hipStream_t st, const float4* vertices, const NormalArgs& a, float4* face_vectors);
// out[2 * i], out[2 * i + 1] = in[2 * i], in[2 * i + 1] with the normal words the rule gives vertex i of the set, i < n, where its row is
// not empty (nothing is stored elsewhere); in: the set's first vertex; out may be `in` itself
hipError_t launch_vertex_normals(hipStream_t st, const float4* in, const NormalArgs& a, const float4* face_vectors, float4* out);

// debug / parity hooks
hipError_t launch_debug_closest(hipStream_t st, const DeviceScene& scene, const float* origins, const float* dirs, uint32_t n, float tmin,
                                float* t, uint32_t* tri, uint32_t* inst, float* u, float* v, uint32_t* overflow, uint32_t overflow_depth);
hipError_t launch_debug_any(hipStream_t st, const DeviceScene& scene, const float* origins, const float* dirs, const float* tmax, uint32_t n,
                            float tmin, uint8_t* hit, uint32_t* overflow, uint32_t overflow_depth);
hipError_t launch_debug_sample_texture(hipStream_t st, const DeviceScene& scene, uint32_t texture, const float* uv2, const float* footprint4,
                                       uint32_t n, float* rgba);
hipError_t launch_debug_detmath(hipStream_t st, int fn, const float* x, const float* y, uint32_t n, float* out);
// from_surface_color (illuminant 0) / from_illuminant_color (1) of device/shading.h on n colours, 16 bins out per colour
hipError_t launch_debug_color_to_spec(hipStream_t st, int illuminant, const float* rgb3, uint32_t n, float* out16);
// bsdf_eval / bsdf_sample / sample_light + light_emission of device/shading.h, one thread per element (uv2: one pair per call; frame9: s, t, n
// stored as given, null = x, y, z); all pointers are device memory
hipError_t launch_debug_bsdf_value(hipStream_t st, const DeviceScene& scene, uint32_t material, const float* wo3, const float* wi3, const float* uv2,
                                   const float* rand1, const float* frame9, uint32_t n, float* value16, float* pdf);
hipError_t launch_debug_bsdf_sample(hipStream_t st, const DeviceScene& scene, uint32_t material, const float* wo3, const float* uv2, const float* rand3,
                                    const float* frame9, uint32_t n, float* wi3, float* value16, float* pdf);
hipError_t launch_debug_light_sample(hipStream_t st, const DeviceScene& scene, uint32_t light, const float* pos3, const float* rand3, uint32_t n,
                                     float scene_radius, float* wi3, float* dist, float* pdf, float* emission16);

}  // namespace glz
