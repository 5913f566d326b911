// The acceleration structure and its update paths (accel.h).
#include "accel.h"

#include <algorithm>
#include <cmath>
#include <cstring>

#include "host_math.h"

namespace glz {

std::vector<TransformPair> transform_pairs(const std::vector<glz_transform>& transforms) {
  std::vector<TransformPair> xf(transforms.size());
  for (size_t i = 0; i < xf.size(); ++i) {
    memcpy(xf[i].o2w, transforms[i].m, 64);
    host::Mat4d inv;
    if (!host::invert(host::Mat4d::from_f32(transforms[i].m), inv)) inv = host::Mat4d::identity();
    inv.to_f32(xf[i].w2o);
  }
  return xf;
}

// DeviceScene::xf_identity: 1 for a transform that is bitwise the identity (-0.0 does not count)
static std::vector<uint32_t> identity_flags(const std::vector<glz_transform>& transforms) {
  std::vector<uint32_t> ident(transforms.size(), 0u);
  for (size_t i = 0; i < ident.size(); ++i) {
    static const float id[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    ident[i] = memcmp(transforms[i].m, id, 64) == 0 ? 1u : 0u;
  }
  return ident;
}

static std::vector<uint32_t> instance_transforms(const std::vector<RTInstance>& instances) {
  std::vector<uint32_t> out(instances.size());
  for (size_t i = 0; i < out.size(); ++i) out[i] = instances[i].transform_id;
  return out;
}

const char* traversal_offsets_exceeded(const TraversalSizes& s) {
  constexpr uint64_t kLimit = 1ull << 32;   // first byte offset that 32 bits do not hold
  auto reaches = [](uint64_t n, uint64_t record) { return n >= (kLimit + record - 1) / record; };   // n * record >= 2^32, without the product
  if (reaches(s.n_nodes, sizeof(BvhNode4))) return "the hierarchy's 4-wide nodes take 2^32 bytes or more (the tracers address them with 32-bit byte offsets)";
  if (reaches(s.n_nodes8, sizeof(BvhNode8))) return "the hierarchy's 8-wide nodes take 2^32 bytes or more (the tracers address them with 32-bit byte offsets)";
  if (reaches(s.n_leaves, sizeof(BvhQuad))) return "the hierarchy's leaf records take 2^32 bytes or more (the tracers address them with 32-bit byte offsets)";
  if (reaches(s.n_instances, sizeof(TlasInstance))) return "the instance records take 2^32 bytes or more (the tracers address them with 32-bit byte offsets)";
  constexpr uint64_t kWords = kLimit / sizeof(uint32_t);   // (each factor below it first: the product cannot wrap)
  if (s.grid_lanes >= kWords || s.overflow_depth >= kWords || s.grid_lanes * s.overflow_depth >= kWords)
    return "the traversal stacks' spill area takes 2^32 bytes or more (the hierarchy is too deep for 32-bit byte offsets)";
  return nullptr;
}

// the structure as built against traversal_offsets_exceeded, with the largest persistent grid the current device is given
bool Accel::offsets_fit(Error& err) const {
  int dev = 0, cus = 256;   // (launch_geometry.h resident_blocks: the same query, the same default)
  hipDeviceProp_t prop;
  if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0) cus = prop.multiProcessorCount;
  const TraversalSizes sizes{d_nodes_.count, d_nodes8_.count, d_quads_.count, d_tlas_instances_.count, (uint64_t)cus * kPersistentBlocksPerCuMax * kTraceBlock, stack_overflow_depth};
  const char* what = traversal_offsets_exceeded(sizes);
  return what ? err.fail(GLZ_E_INVALID_DATA, what) : true;
}

void Accel::describe(DeviceScene& dev) const {
  dev.bvh_nodes = d_nodes_.ptr;
  dev.bvh_top = d_top_.ptr;
  dev.bvh_grid = grid_;
  dev.bvh_tris = d_tris_.ptr;
  dev.bvh_quads = d_quads_.ptr;   // world space, or the meshes' leaf records concatenated
  dev.shade_tris = d_shade_tris_.ptr;
  dev.xf_identity = d_xf_identity_.ptr;
  dev.n_world_tris = n_world_tris_;
  dev.two_level = two_level_ ? 1u : 0u;
  if (two_level_) {   // (the two-level tracer walks 4-wide nodes only, and takes the alpha test's material from the instance)
    dev.tlas_nodes = d_nodes_.ptr;
    dev.tlas_instances = d_tlas_instances_.ptr;
  } else {
    dev.bvh_nodes8 = d_nodes8_.ptr;
    if (alpha_ready_) dev.alpha_recs = d_alpha_recs_.ptr;
  }
}

void Accel::describe(glz_scene_info& info) const {
  info.bvh_nodes = info_.bvh_nodes;
  info.bvh_nodes8 = info_.bvh_nodes8;
  info.bvh_depth = info_.bvh_depth;
  info.bvh_sah_cost = info_.bvh_sah_cost;
  info.build_ms = info_.build_ms;
  for (int k = 0; k < 3; ++k) {
    info.bounds_min[k] = info_.bounds_min[k];
    info.bounds_max[k] = info_.bounds_max[k];
    info.bvh_grid_lo[k] = info_.bvh_grid_lo[k];
    info.bvh_grid_cell[k] = info_.bvh_grid_cell[k];
  }
  info.as_levels = info_.as_levels;
  info.n_as_triangles = info_.n_as_triangles;
  info.as_bytes = info_.as_bytes;
}

// Two-level structure (types.h TlasInstance; acceleration.rs:319-345: a BLAS per mesh, a TLAS over the instances).  The meshes'
// hierarchies are built by the ordinary builder over ONE pseudo-instance with the identity transform (object space = its "world"),
// the top level by the same builder over the instances' world boxes (HierarchyInputs::given_lo).  Memory is O(meshes + instances).
bool Accel::build_two_level(const Sources& s, Error& err) {
  hipStream_t st = s.stream;
  const Geometry& g = s.geometry;
  StreamTimer timer;
  if (!timer.start(st, err)) return false;
  h_mesh_ranges.clear();
  plans_.clear();   // (the meshes' hierarchies are new)
  // ---- unique meshes (index ranges) ----
  std::vector<uint32_t> mesh_of;
  std::vector<MeshBuild> meshes;
  uint64_t total_tris = 0;
  for (const std::pair<uint32_t, uint32_t>& range : unique_meshes(g.h_instances, mesh_of)) {
    meshes.emplace_back();
    meshes.back().mesh.index_offset = range.first;
    meshes.back().mesh.index_count = range.second;
    meshes.back().range.tri_base = (uint32_t)total_tris;
    total_tris += range.second / 3u;
  }
  if (total_tris >= 0x3FFFFFFFull) return err.fail(GLZ_E_UNSUPPORTED, "more than 2^30 mesh triangles");
  const uint32_t nt = (uint32_t)total_tris;
  d_nodes_.release();
  if (!hip_ok(d_tris_.alloc((size_t)nt + 1), "alloc BVH triangles", err)) return false;
  if (!hip_ok(hipMemsetAsync(d_tris_.ptr + nt, 0, sizeof(BvhTri), st), "clear BVH triangle padding", err)) return false;
  if (!hip_ok(d_shade_tris_.alloc((size_t)nt * 8), "alloc shading records", err)) return false;
  // helpers of the per-mesh builds: an identity transform, an opaque material (the opacity flag is per instance here)
  DeviceBuffer<TransformPair> d_ident;
  DeviceBuffer<RTMaterial> d_opaque;
  DeviceBuffer<RTInstance> d_pseudo;
  DeviceBuffer<uint32_t> d_zero, d_one;
  {
    TransformPair ident{};
    for (int k = 0; k < 4; ++k) ident.o2w[5 * k] = ident.w2o[5 * k] = 1.0f;
    RTMaterial opaque{};
    const uint32_t zero = 0u, one = 1u;
    if (!hip_ok(d_ident.upload(&ident, 1, st), "upload", err) || !hip_ok(d_opaque.upload(&opaque, 1, st), "upload", err) ||
        !hip_ok(d_zero.upload(&zero, 1, st), "upload", err) || !hip_ok(d_one.upload(&one, 1, st), "upload", err) || !hip_ok(d_pseudo.alloc(1), "alloc", err))
      return false;
    if (!hip_ok(hipStreamSynchronize(st), "upload", err)) return false;
  }
  tl_mesh_depth_ = 0;
  for (MeshBuild& m : meshes) {
    const uint32_t n = m.mesh.index_count / 3u;
    if (n == 0) continue;
    const RTInstance pseudo{m.mesh.index_offset, m.mesh.index_count, 0u, 0u};
    if (!hip_ok(hipMemcpyAsync(d_pseudo.ptr, &pseudo, sizeof(pseudo), hipMemcpyHostToDevice, st), "upload", err) || !hip_ok(hipStreamSynchronize(st), "upload", err))
      return false;
    HierarchyInputs in{g.vertices.ptr, g.indices.ptr, d_pseudo.ptr, d_zero.ptr, 1u, d_ident.ptr, d_opaque.ptr, n, build_opts_.builder, build_opts_.pair_area_ratio};
    in.emit_quads = true;   // 64-byte leaf records (object space here), leaf links ~leaf number relative to the mesh
    HierarchyOutputs out{};
    DeviceBuffer<BvhTri> tris;
    if (!hip_ok(tris.alloc((size_t)n + 1), "alloc mesh triangles", err)) return false;
    out.tris = tris.ptr;
    if (!hip_ok(build_hierarchy(st, in, out), "mesh hierarchy", err)) return false;
    m.nodes = std::move(out.nodes);
    m.quads = std::move(out.quads);   // the mesh's leaf records (object space)
    m.mesh.grid = out.grid;
    for (int k = 0; k < 3; ++k) { m.mesh.lo[k] = out.bounds_lo[k]; m.mesh.hi[k] = out.bounds_hi[k]; }
    tl_mesh_depth_ = std::max(tl_mesh_depth_, out.depth);
    // the mesh's triangles and per-object-triangle shading records go to their place in the concatenated arrays
    if (!hip_ok(hipMemcpyAsync(d_tris_.ptr + m.range.tri_base, tris.ptr, sizeof(BvhTri) * n, hipMemcpyDeviceToDevice, st), "copy mesh triangles", err) ||
        !hip_ok(launch_shade_records(st, n, tris.ptr, d_pseudo.ptr, g.indices.ptr, g.vertices.ptr, g.derivatives.ptr, d_one.ptr,
                                     d_shade_tris_.ptr + 8 * (size_t)m.range.tri_base), "k_shade_records", err) ||
        !hip_ok(hipStreamSynchronize(st), "mesh hierarchy", err))
      return false;
  }
  // ---- where each mesh's nodes and leaf records go: one array each (TlasInstance::node_base / quad_base); the nodes follow a top
  // level that does not exist yet ----
  uint32_t total_leaves = 0;
  tl_top_nodes_ = 0;
  uint32_t at = 0;
  for (MeshBuild& m : meshes) {
    m.range.node_base = at;
    m.range.n_nodes = (uint32_t)m.nodes.count;
    m.range.quad_base = total_leaves;
    at += m.range.n_nodes ? m.range.n_nodes : 1u;   // a mesh without triangles gets one node without children: entering it finds nothing
    total_leaves += (uint32_t)m.quads.count;
  }
  d_quads_.release();
  if (!hip_ok(d_quads_.alloc((size_t)total_leaves + 1), "alloc leaf records", err) ||
      !hip_ok(hipMemsetAsync(d_quads_.ptr + total_leaves, 0, sizeof(BvhQuad), st), "clear leaf record padding", err))
    return false;
  for (const MeshBuild& m : meshes)
    if (m.quads.count && !hip_ok(hipMemcpyAsync(d_quads_.ptr + m.range.quad_base, m.quads.ptr, sizeof(BvhQuad) * m.quads.count, hipMemcpyDeviceToDevice, st), "copy leaf records", err))
      return false;
  // ---- what the top level needs of each mesh, kept for rebuild() ----
  tl_meshes_.clear();
  for (const MeshBuild& m : meshes) {
    tl_meshes_.push_back(m.mesh);
    h_mesh_ranges.push_back(m.range);
  }
  tl_mesh_of_ = mesh_of;
  tl_points_ready_ = false;
  // ---- instance boxes (host_instance_boxes), then the top level over them ----
  const size_t ni = g.h_instances.size();
  std::vector<float4> blo, bhi;
  host_instance_boxes(tl_mesh_of_, instance_transforms(g.h_instances), box_meshes(s.data), s.data.transforms, kExactBoxBudget, blo, bhi);
  DeviceBuffer<float4> d_blo, d_bhi;
  if (!hip_ok(d_blo.upload(blo.data(), ni, st), "upload instance boxes", err) || !hip_ok(d_bhi.upload(bhi.data(), ni, st), "upload instance boxes", err) ||
      !hip_ok(hipStreamSynchronize(st), "upload instance boxes", err))
    return false;
  return assemble_top_level(s, d_blo.ptr, d_bhi.ptr, blo, bhi, &meshes, timer, err);
}

// Everything from "the instance boxes are on the device" onwards, for a new scene and for moved instances alike: the hierarchy over
// the boxes, its nodes in front of the meshes' nodes in one array, the instance records in its leaf order, the top table, info.
// h_lo / h_hi: host copies of the boxes; empty = read back here.  built: the meshes' nodes as a build has just left them (their
// place in the array: h_mesh_ranges, behind tl_top_nodes_ = 0 top nodes), or null = they sit in d_nodes_ behind the old top level.
// timer: started by the caller, where info.build_ms is to begin.
bool Accel::assemble_top_level(const Sources& s, const float4* d_lo, const float4* d_hi, std::vector<float4>& h_lo, std::vector<float4>& h_hi,
                               const std::vector<MeshBuild>* built, StreamTimer& timer, Error& err) {
  hipStream_t st = s.stream;
  const size_t ni = s.geometry.h_instances.size();
  DeviceBuffer<BvhTri> top_tris;
  HierarchyOutputs top{};
  if (!hip_ok(top_tris.alloc(ni + 1), "alloc", err)) return false;
  {
    HierarchyInputs in{nullptr, nullptr, nullptr, nullptr, 0u, nullptr, nullptr, (uint32_t)ni, build_opts_.builder, 0.0f};
    in.given_lo = d_lo;
    in.given_hi = d_hi;
    top.tris = top_tris.ptr;
    if (!hip_ok(build_hierarchy(st, in, top), "instance hierarchy", err)) return false;
  }
  // ---- one node array: top level first, then the meshes (moved as they are when the top level's size changes) ----
  const MeshRange& last = h_mesh_ranges.back();   // (a two-level scene has a mesh)
  const uint32_t old_top = tl_top_nodes_, new_top = (uint32_t)top.nodes.count;
  const uint32_t mesh_nodes = last.node_base + (last.n_nodes ? last.n_nodes : 1u) - old_top, n_nodes = new_top + mesh_nodes;
  if (n_nodes >= (uint32_t)kBvhTopFlag) return err.fail(GLZ_E_UNSUPPORTED, "more than 2^30 BVH nodes");
  DeviceBuffer<BvhNode4> fresh;
  const bool in_place = !built && new_top == old_top;
  if (!in_place && !hip_ok(fresh.alloc(n_nodes), "alloc nodes", err)) return false;
  BvhNode4* nodes = in_place ? d_nodes_.ptr : fresh.ptr;
  bool ok = !new_top || hip_ok(hipMemcpyAsync(nodes, top.nodes.ptr, sizeof(BvhNode4) * new_top, hipMemcpyDeviceToDevice, st), "copy nodes", err);
  if (built) {
    static const BvhNode4 childless = childless_node4();   // (static: the copy below is asynchronous)
    for (const MeshBuild& m : *built) {
      BvhNode4* to = nodes + new_top + m.range.node_base;
      if (ok && m.nodes.count) ok = hip_ok(hipMemcpyAsync(to, m.nodes.ptr, sizeof(BvhNode4) * m.nodes.count, hipMemcpyDeviceToDevice, st), "copy nodes", err);
      if (ok && !m.nodes.count) ok = hip_ok(hipMemcpyAsync(to, &childless, sizeof(BvhNode4), hipMemcpyHostToDevice, st), "copy nodes", err);
    }
  } else if (!in_place && ok) {
    ok = hip_ok(hipMemcpyAsync(nodes + new_top, d_nodes_.ptr + old_top, sizeof(BvhNode4) * mesh_nodes, hipMemcpyDeviceToDevice, st), "move mesh nodes", err);
  }
  // instance records in the top level's leaf order
  std::vector<BvhTri> order(ni);
  if (ok) ok = hip_ok(hipMemcpyAsync(order.data(), top_tris.ptr, sizeof(BvhTri) * ni, hipMemcpyDeviceToHost, st), "read instance order", err);
  if (h_lo.empty()) {
    h_lo.resize(ni);
    h_hi.resize(ni);
    if (ok) ok = hip_ok(hipMemcpyAsync(h_lo.data(), d_lo, sizeof(float4) * ni, hipMemcpyDeviceToHost, st), "read instance boxes", err);
    if (ok) ok = hip_ok(hipMemcpyAsync(h_hi.data(), d_hi, sizeof(float4) * ni, hipMemcpyDeviceToHost, st), "read instance boxes", err);
  }
  if (!hip_ok(hipStreamSynchronize(st), "top level", err) || !ok) return false;
  if (!in_place) {
    d_nodes_ = std::move(fresh);
    for (MeshRange& r : h_mesh_ranges) r.node_base = r.node_base - old_top + new_top;
  }
  tl_top_nodes_ = new_top;
  if (!write_top_records(s, order, instance_reach(h_lo, h_hi), err)) return false;
  if (!d_top_.ptr && !hip_ok(d_top_.alloc(kBvhTopNodes), "alloc BVH top table", err)) return false;
  if (!hip_ok(launch_top_table(st, d_nodes_.ptr, new_top, d_top_.ptr), "k_top_table", err)) return false;   // unused by the two-level tracer, kept valid
  timer.stop(st);
  if (!hip_ok(hipStreamSynchronize(st), "top level", err)) return false;
  finish_two_level(s, top, timer.ms());
  return offsets_fit(err);
}

// The TlasInstance records in the top level's leaf order (`order`: the top level's leaves, world_id = instance), and the transform
// flags.  `reach`: instance_reach of the instance boxes the top level was built over.
bool Accel::write_top_records(const Sources& s, const std::vector<BvhTri>& order, double reach, Error& err) {
  hipStream_t st = s.stream;
  const size_t ni = s.geometry.h_instances.size();
  std::vector<TlasInstance> recs(ni);
  const std::vector<TransformPair> xf = transform_pairs(s.data.transforms);
  for (size_t slot = 0; slot < ni; ++slot) {
    const uint32_t i = order[slot].world_id;   // the box this leaf was built from
    const RTInstance& in = s.geometry.h_instances[i];
    const TlMesh& m = tl_meshes_[tl_mesh_of_[i]];
    const MeshRange& mr = h_mesh_ranges[tl_mesh_of_[i]];
    const TransformPair& T = xf[in.transform_id];
    TlasInstance r{};
    for (int row = 0; row < 3; ++row)
      for (int col = 0; col < 4; ++col) r.w2o[4 * row + col] = T.w2o[4 * col + row];   // rows of the column-major inverse
    memcpy(r.o2w, T.o2w, 64);
    r.grid = m.grid;
    // slack of the object-space box tests: rounding of the transformed ray (relative to where in the world it can be) and of
    // the triangle's world position, taken back to object units; generous (x 32)
    double wnorm = 0.0, tr = 0.0, objmax = 0.0;
    for (int row = 0; row < 3; ++row) {
      wnorm = std::max(wnorm, std::fabs((double)r.w2o[4 * row]) + std::fabs((double)r.w2o[4 * row + 1]) + std::fabs((double)r.w2o[4 * row + 2]));
      tr = std::max(tr, std::fabs((double)r.w2o[4 * row + 3]));
      objmax = std::max({objmax, std::fabs((double)m.lo[row]), std::fabs((double)m.hi[row])});
    }
    const double eps = 1.1920929e-7;
    // (in object units: the tracer turns it into cells of each axis -- a thin mesh has tiny cells across its thin side, and the pad
    // that side needs, taken for all three, would make every box of the mesh as wide as the mesh)
    r.slack = (float)(32.0 * eps * (wnorm * reach + tr + objmax));
    r.w2o_norm = (float)wnorm;   // the tracer adds 32 eps wnorm |o|_1 per ray: origins far outside the scene's bounds
    r.node_base = mr.node_base;
    r.tri_base = mr.tri_base;
    r.quad_base = mr.quad_base;
    r.world_base = s.geometry.h_inst_base[i];
    r.instance = i;
    r.non_opaque = s.tables.h_materials[in.material_id].opacity != 0 ? 1u : 0u;
    recs[slot] = r;
  }
  if (!hip_ok(d_tlas_instances_.upload(recs.data(), ni, st), "upload instance records", err)) return false;
  const std::vector<uint32_t> ident = identity_flags(s.data.transforms);
  if (!hip_ok(d_xf_identity_.upload(ident.data(), ident.size(), st), "upload transform flags", err)) return false;
  return hip_ok(hipStreamSynchronize(st), "upload instance records", err);   // the staging vectors above must outlive the copies
}

// info and stack bound of a two-level scene whose node array (top level first) and records are in place
void Accel::finish_two_level(const Sources& s, const HierarchyOutputs& top, float build_ms) {
  const uint32_t n_nodes = (uint32_t)d_nodes_.count, nt = (uint32_t)(d_tris_.count - 1), ni = (uint32_t)s.geometry.h_instances.size();
  info_.bvh_nodes = n_nodes;
  info_.bvh_depth = top.depth + tl_mesh_depth_;
  info_.bvh_sah_cost = top.sah;
  info_.build_ms = build_ms;
  for (int k = 0; k < 3; ++k) {
    info_.bounds_min[k] = top.bounds_lo[k];
    info_.bounds_max[k] = top.bounds_hi[k];
    info_.bvh_grid_lo[k] = top.grid.lo[k];
    info_.bvh_grid_cell[k] = top.grid.cell[k];
  }
  // both levels' entries and one exit marker share the stack
  const uint32_t stack_bound = 3u * (top.depth + tl_mesh_depth_) + 2u;
  stack_overflow_depth = stack_bound > (uint32_t)kTraversalLdsStack ? stack_bound - kTraversalLdsStack + 1 : 1;
  grid_ = top.grid;
  two_level_ = true;
  d_nodes8_.release();   // (the two-level tracer walks 4-wide nodes only)
  info_.bvh_nodes8 = 0;
  info_.as_levels = 2;
  info_.n_as_triangles = nt;
  info_.as_bytes = (uint64_t)n_nodes * sizeof(BvhNode4) + (uint64_t)(nt + 1) * sizeof(BvhTri) + (uint64_t)nt * 128u + (uint64_t)ni * sizeof(TlasInstance) +
                   (uint64_t)d_quads_.count * sizeof(BvhQuad);
}

bool Accel::build(const BuildOptions& opts, const Sources& s, Error& err) {
  build_opts_ = opts;
  if (!build_bvh(s, err)) return false;
  build_opts_.as_levels = (int)info_.as_levels;   // the shape built
  return true;
}

bool Accel::build_bvh(const Sources& s, Error& err) {
  const Geometry& g = s.geometry;
  two_level_ = false;
  alpha_ready_ = false;
  plans_.clear();   // a refit plan belongs to the structure it was made for
  n_world_tris_ = (uint32_t)g.n_world_triangles;
  // instanced scenes keep one hierarchy per mesh (acceleration.rs:319-345) instead of one over every instanced triangle
  {
    uint64_t unique = 0;
    std::vector<uint32_t> mesh_of;
    for (const std::pair<uint32_t, uint32_t>& range : unique_meshes(g.h_instances, mesh_of)) unique += range.second / 3u;
    const bool wanted = build_opts_.as_levels == 2 || (build_opts_.as_levels == 0 && unique > 0 && g.n_world_triangles > 4 * unique);
    if (wanted && g.n_world_triangles > 0) return build_two_level(s, err);
  }
  hipStream_t st = s.stream;
  const uint32_t n = n_world_tris_;
  d_nodes_.release();
  if (!hip_ok(d_tris_.alloc((size_t)n + 1), "alloc BVH triangles", err)) return false;   // + 1: the tracer loads a leaf's partner slot unconditionally
  if (!hip_ok(hipMemsetAsync(d_tris_.ptr + n, 0, sizeof(BvhTri), st), "clear BVH triangle padding", err)) return false;
  HierarchyInputs in{g.vertices.ptr, g.indices.ptr, g.instances.ptr, g.inst_base.ptr, (uint32_t)g.h_instances.size(), g.transforms.ptr,
                     s.tables.materials(), n, build_opts_.builder, build_opts_.pair_area_ratio};
  in.emit_quads = true;   // the flattened tracer reads one 64-byte record per leaf (types.h BvhQuad); leaf links are ~leaf number
  in.emit_wide8 = true;   // ... and a small tile share the same hierarchy eight wide (types.h BvhNode8, k_trace8)
  HierarchyOutputs out{};
  out.tris = d_tris_.ptr;
  d_quads_.release();
  d_nodes8_.release();
  StreamTimer timer;
  if (!timer.start(st, err)) return false;
  const hipError_t be = build_hierarchy(st, in, out);
  timer.stop(st);
  const float ms = timer.ms();
  if (!hip_ok(be, "hierarchy build", err)) return false;
  d_quads_ = std::move(out.quads);
  d_nodes8_ = std::move(out.nodes8);
  d_nodes_ = std::move(out.nodes);   // allocated by the build once the number of 4-wide nodes is known
  const uint32_t n_nodes = (uint32_t)d_nodes_.count;
  info_.bvh_nodes = n_nodes;
  info_.bvh_depth = out.depth;
  info_.bvh_sah_cost = out.sah;
  info_.build_ms = ms;
  for (int k = 0; k < 3; ++k) {
    info_.bounds_min[k] = out.bounds_lo[k];
    info_.bounds_max[k] = out.bounds_hi[k];
  }
  // traversal stack: kTraversalLdsStack levels live in LDS, the rest spills to a per-lane HBM area
  // (a 4-wide visit pushes up to three siblings, so the bound is 3 entries per level)
  const uint32_t stack_bound = std::max(3u * out.depth, 7u * out.depth8) + 1u;   // (an 8-wide visit pushes up to seven)
  stack_overflow_depth = stack_bound > (uint32_t)kTraversalLdsStack ? stack_bound - kTraversalLdsStack + 1 : 1;
  if (n_nodes >= (uint32_t)kBvhTopFlag) return err.fail(GLZ_E_UNSUPPORTED, "more than 2^30 BVH nodes");
  if (!offsets_fit(err)) return false;
  // top levels of the tree for the tracers' LDS staging
  if (!d_top_.ptr && !hip_ok(d_top_.alloc(kBvhTopNodes), "alloc BVH top table", err)) return false;
  if (!hip_ok(launch_top_table(st, d_nodes_.ptr, n_nodes, d_top_.ptr), "k_top_table", err)) return false;
  info_.bvh_nodes8 = (uint32_t)d_nodes8_.count;
  grid_ = out.grid;
  for (int k = 0; k < 3; ++k) {
    info_.bvh_grid_lo[k] = out.grid.lo[k];
    info_.bvh_grid_cell[k] = out.grid.cell[k];
  }
  // per-leaf shading records (the identity flags let k_shade skip the object->world transform exactly)
  const std::vector<uint32_t> ident = identity_flags(s.data.transforms);
  if (!hip_ok(d_xf_identity_.upload(ident.data(), ident.size(), st), "upload transform flags", err)) return false;
  if (!hip_ok(d_shade_tris_.alloc((size_t)n * 8), "alloc shading records", err)) return false;
  if (!hip_ok(launch_shade_records(st, n, d_tris_.ptr, g.instances.ptr, g.indices.ptr, g.vertices.ptr, g.derivatives.ptr, d_xf_identity_.ptr,
                                   d_shade_tris_.ptr), "k_shade_records", err))
    return false;
  if (!hip_ok(hipStreamSynchronize(st), "shading records", err)) return false;
  n_shade_slots_ = n;
  if (!build_alpha_records(s, err)) return false;
  info_.as_levels = 1;
  info_.n_as_triangles = n;
  info_.as_bytes = (uint64_t)n_nodes * sizeof(BvhNode4) + (uint64_t)(n + 1) * sizeof(BvhTri) + (uint64_t)n * 128u + (uint64_t)d_quads_.count * sizeof(BvhQuad) +
                   (uint64_t)info_.bvh_nodes8 * sizeof(BvhNode8);
  return true;
}

bool Accel::build_alpha_records(const Sources& s, Error& err) {
  alpha_ready_ = false;
  if (two_level_ || !s.tables.has_non_opaque() || n_shade_slots_ == 0 || !d_shade_tris_.ptr) return true;
  if (!hip_ok(d_alpha_recs_.alloc((size_t)n_shade_slots_ * 3), "alloc alpha records", err)) return false;
  if (!hip_ok(launch_alpha_records(s.stream, n_shade_slots_, d_shade_tris_.ptr, s.tables.materials(), s.textures.descriptors(), d_alpha_recs_.ptr), "k_alpha_records", err))
    return false;
  if (!hip_ok(hipStreamSynchronize(s.stream), "alpha records", err)) return false;
  alpha_ready_ = true;
  return true;
}

// ---- moving instances ------------------------------------------------------------------------------------------------------------
std::vector<InstanceBoxMesh> Accel::box_meshes(const SceneData& data) const {
  std::vector<std::pair<uint32_t, uint32_t>> ranges;
  for (const TlMesh& m : tl_meshes_) ranges.emplace_back(m.index_offset, m.index_count);
  std::vector<std::vector<float>> pts = mesh_points(data, ranges);
  std::vector<InstanceBoxMesh> out(tl_meshes_.size());
  for (size_t m = 0; m < out.size(); ++m) {
    for (int k = 0; k < 3; ++k) {
      out[m].lo[k] = tl_meshes_[m].lo[k];
      out[m].hi[k] = tl_meshes_[m].hi[k];
    }
    out[m].points = std::move(pts[m]);
  }
  return out;
}

// The device side of host_instance_boxes for the scene's current transforms (Geometry::transforms), into d_box_lo_ / d_box_hi_.
bool Accel::device_instance_boxes(const Sources& s, uint64_t budget, Error& err) {
  hipStream_t st = s.stream;
  const std::vector<RTInstance>& instances = s.geometry.h_instances;
  const size_t nm = tl_meshes_.size(), ni = instances.size();
  if (!tl_points_ready_) {
    const std::vector<InstanceBoxMesh> bm = box_meshes(s.data);
    std::vector<float4> pts, mlo(nm), mhi(nm);
    tl_point_base_.assign(nm, 0);
    tl_point_count_.assign(nm, 0);
    for (size_t m = 0; m < nm; ++m) {
      tl_point_base_[m] = (uint32_t)pts.size();
      tl_point_count_[m] = bm[m].points.size() / 3;
      for (size_t p = 0; p + 2 < bm[m].points.size(); p += 3) pts.push_back(make_float4(bm[m].points[p], bm[m].points[p + 1], bm[m].points[p + 2], 0.0f));
      mlo[m] = make_float4(bm[m].lo[0], bm[m].lo[1], bm[m].lo[2], 0.0f);
      mhi[m] = make_float4(bm[m].hi[0], bm[m].hi[1], bm[m].hi[2], 0.0f);
    }
    for (size_t m = 0; m < nm; ++m)   // the corners, in host_instance_boxes' order, after every mesh's points
      for (int c = 0; c < 8; ++c)
        pts.push_back(make_float4((c & 1) ? bm[m].hi[0] : bm[m].lo[0], (c & 2) ? bm[m].hi[1] : bm[m].lo[1], (c & 4) ? bm[m].hi[2] : bm[m].lo[2], 0.0f));
    if (pts.size() >= 0xFFFFFFFFull) return err.fail(GLZ_E_UNSUPPORTED, "more than 2^32 mesh vertices");
    if (!hip_ok(d_tl_points_.upload(pts.data(), pts.size(), st), "upload mesh points", err) ||
        !hip_ok(d_tl_mesh_lo_.upload(mlo.data(), nm, st), "upload mesh boxes", err) || !hip_ok(d_tl_mesh_hi_.upload(mhi.data(), nm, st), "upload mesh boxes", err) ||
        !hip_ok(hipStreamSynchronize(st), "upload mesh points", err))
      return false;
    tl_points_ready_ = true;
  }
  // work items: an exact instance's points in chunks of one wave's share, the others' eight corners (exact_box_instances chooses, as on the host)
  constexpr uint32_t kChunk = 64u * 32u;
  const uint32_t corner_base = (uint32_t)(d_tl_points_.count - 8 * nm);
  const std::vector<uint8_t> exact = exact_box_instances(tl_mesh_of_, tl_point_count_, budget);
  std::vector<InstanceBoxItem> items;
  std::vector<uint32_t> first(ni + 1);
  for (size_t i = 0; i < ni; ++i) {
    first[i] = (uint32_t)items.size();
    const uint32_t m = tl_mesh_of_[i], t = instances[i].transform_id;
    if (!exact[i]) {
      items.push_back(InstanceBoxItem{t, m, corner_base + 8u * m, 8u});
      continue;
    }
    for (uint64_t p = 0; p < tl_point_count_[m]; p += kChunk)
      items.push_back(InstanceBoxItem{t, m, tl_point_base_[m] + (uint32_t)p, (uint32_t)std::min<uint64_t>(kChunk, tl_point_count_[m] - p)});
  }
  first[ni] = (uint32_t)items.size();
  DeviceBuffer<InstanceBoxItem> d_items;
  DeviceBuffer<uint32_t> d_first;
  DeviceBuffer<double> d_partial;
  if (!hip_ok(d_items.upload(items.data(), items.size(), st), "upload box items", err) || !hip_ok(d_first.upload(first.data(), first.size(), st), "upload box items", err) ||
      !hip_ok(d_partial.alloc(6 * items.size()), "alloc box partials", err))
    return false;
  if (d_box_lo_.count != ni && (!hip_ok(d_box_lo_.alloc(ni), "alloc instance boxes", err) || !hip_ok(d_box_hi_.alloc(ni), "alloc instance boxes", err))) return false;
  StreamTimer timer;
  if (!timer.start(st, err)) return false;
  if (!hip_ok(launch_instance_boxes(st, (uint32_t)items.size(), d_items.ptr, d_tl_points_.ptr, s.geometry.transforms.ptr, d_partial.ptr, (uint32_t)ni, d_first.ptr,
                                    d_tl_mesh_lo_.ptr, d_tl_mesh_hi_.ptr, d_box_lo_.ptr, d_box_hi_.ptr), "k_instance_boxes", err))
    return false;
  timer.stop(st);
  if (!hip_ok(hipStreamSynchronize(st), "instance boxes", err)) return false;   // the staging vectors and scratch above must outlive the kernels
  box_kernel_ms = timer.ms();
  return true;
}

bool Accel::instance_boxes(const Sources& s, bool on_device, uint64_t budget, std::vector<float4>& lo, std::vector<float4>& hi, Error& err) {
  lo.clear();
  hi.clear();
  if (!two_level_) return false;
  if (!on_device) {
    host_instance_boxes(tl_mesh_of_, instance_transforms(s.geometry.h_instances), box_meshes(s.data), s.data.transforms, budget, lo, hi);
    return true;
  }
  if (!device_instance_boxes(s, budget, err)) return false;
  lo.resize(s.geometry.h_instances.size());
  hi.resize(s.geometry.h_instances.size());
  return hip_ok(hipMemcpy(lo.data(), d_box_lo_.ptr, sizeof(float4) * lo.size(), hipMemcpyDeviceToHost), "read instance boxes", err) &&
         hip_ok(hipMemcpy(hi.data(), d_box_hi_.ptr, sizeof(float4) * hi.size(), hipMemcpyDeviceToHost), "read instance boxes", err);
}

bool Accel::rebuild(const Sources& s, Error& err) {
  // a flattened scene's world triangles depend on every transform: the whole structure again, with the options it was built with
  if (!two_level_) return build_bvh(s, err) && hip_ok(hipStreamSynchronize(s.stream), "update_transforms", err);
  // The top level again, over the instance boxes of the current transforms; the meshes' hierarchies, leaf records and shading records
  // stay where they are (their links are relative to TlasInstance::node_base / quad_base / tri_base).
  StreamTimer timer;
  if (!timer.start(s.stream, err)) return false;
  if (!device_instance_boxes(s, kExactBoxBudget, err)) return false;
  std::vector<float4> blo, bhi;   // read back with the leaf order
  return assemble_top_level(s, d_box_lo_.ptr, d_box_hi_.ptr, blo, bhi, nullptr, timer, err);
}

// ---- deforming meshes ------------------------------------------------------------------------------------------------------------
// The nodes of one width grouped by height above the leaves: order (nodes of height 0 first) and the offsets of the levels in it.
// Depth-first numbering puts every parent before its children, so one pass from the last node to the first knows the children's heights.
static bool level_lists(const uint32_t* words, uint32_t n_nodes, uint32_t n_leaves, int width, std::vector<uint32_t>& order, std::vector<uint32_t>& first) {
  std::vector<uint32_t> height(n_nodes, 0u);
  uint32_t top = 0;
  for (uint32_t i = n_nodes; i-- > 0;) {
    const uint32_t* link = words + (size_t)i * 4 * width + 3 * width;
    for (int k = 0; k < width; ++k) {
      const int l = (int)link[k];
      if (l == kBvhEmptyChild) continue;
      if (l < 0 ? (uint32_t)~l >= n_leaves : ((uint32_t)l <= i || (uint32_t)l >= n_nodes)) return false;   // (what the kernels index with)
      if (l < 0) continue;
      height[i] = std::max(height[i], height[l] + 1u);
    }
    top = std::max(top, height[i]);
  }
  first.assign(top + 2, 0u);
  for (uint32_t i = 0; i < n_nodes; ++i) ++first[height[i] + 1];
  for (uint32_t h = 0; h <= top; ++h) first[h + 1] += first[h];
  order.resize(n_nodes);
  std::vector<uint32_t> at(first.begin(), first.end() - 1);
  for (uint32_t i = 0; i < n_nodes; ++i) order[at[height[i]]++] = i;
  return true;
}

bool Accel::make_plan(hipStream_t st, const RefitTarget& t, uint32_t n_leaves, RefitPlan& p, Error& err) {
  p.n_leaves = n_leaves;
  if (!hip_ok(alloc_each(n_leaves, p.leaf_lo, p.leaf_hi), "alloc refit leaf boxes", err)) return false;
  if (n_leaves < 2) return true;   // one leaf: one node that spans the grid whatever the leaf's box is; nothing to fit
  std::vector<uint32_t> order;
  std::vector<BvhNode4> h4(t.n_nodes);
  if (!hip_ok(hipMemcpy(h4.data(), t.nodes, sizeof(BvhNode4) * t.n_nodes, hipMemcpyDeviceToHost), "read nodes", err)) return false;
  if (!level_lists(h4[0].w, t.n_nodes, n_leaves, 4, order, p.first4)) return err.fail(GLZ_E_UNSUPPORTED, "refit: the nodes are not as the builder numbers them");
  if (!hip_ok(p.order4.upload(order.data(), order.size(), st), "upload refit plan", err) || !hip_ok(alloc_each(t.n_nodes, p.lo4, p.hi4), "alloc refit node boxes", err) ||
      !hip_ok(hipStreamSynchronize(st), "upload refit plan", err))
    return false;
  if (!t.n_nodes8) return true;
  std::vector<BvhNode8> h8(t.n_nodes8);
  if (!hip_ok(hipMemcpy(h8.data(), t.nodes8, sizeof(BvhNode8) * t.n_nodes8, hipMemcpyDeviceToHost), "read 8-wide nodes", err)) return false;
  if (!level_lists(h8[0].w, t.n_nodes8, n_leaves, 8, order, p.first8)) return err.fail(GLZ_E_UNSUPPORTED, "refit: the 8-wide nodes are not as the builder numbers them");
  return hip_ok(p.order8.upload(order.data(), order.size(), st), "upload refit plan", err) && hip_ok(alloc_each(t.n_nodes8, p.lo8, p.hi8), "alloc refit node boxes", err) &&
         hip_ok(hipStreamSynchronize(st), "upload refit plan", err);
}

Accel::RefitTarget Accel::refit_target(const Sources& s, size_t plan) const {
  if (!two_level_)
    return RefitTarget{d_nodes_.ptr, (uint32_t)d_nodes_.count, d_nodes8_.ptr, (uint32_t)d_nodes8_.count, d_quads_.ptr, d_tris_.ptr, s.geometry.instances.ptr,
                       s.geometry.transforms.ptr};
  const MeshRange& r = h_mesh_ranges[plan];
  return RefitTarget{d_nodes_.ptr + r.node_base, r.n_nodes, nullptr, 0u, d_quads_.ptr + r.quad_base, d_tris_.ptr + r.tri_base, d_tl_pseudo_.ptr + plan, d_tl_ident_.ptr};
}

// One hierarchy under the vertices as they are on the device: leaves, fit, (write) grid and quantisation, the box-area sum into p.area.
bool Accel::refit(hipStream_t st, const Sources& s, const RefitTarget& t, RefitPlan& p, bool write, RefitResult& out, Error& err) {
  const Geometry& g = s.geometry;
  if (!hip_ok(launch_refit_leaves(st, g.vertices.ptr, g.indices.ptr, t.instances, t.transforms, p.n_leaves, t.quads, t.tris, p.leaf_lo.ptr, p.leaf_hi.ptr), "k_refit_leaves", err))
    return false;
  const bool fit = p.n_leaves >= 2;
  const RefitNodes n4{4, t.nodes, t.n_nodes, p.order4.ptr, p.first4, p.leaf_lo.ptr, p.leaf_hi.ptr, p.lo4.ptr, p.hi4.ptr};
  const RefitNodes n8{8, t.nodes8, t.n_nodes8, p.order8.ptr, p.first8, p.leaf_lo.ptr, p.leaf_hi.ptr, p.lo8.ptr, p.hi8.ptr};
  const float4 *root_lo = fit ? p.lo4.ptr : p.leaf_lo.ptr, *root_hi = fit ? p.hi4.ptr : p.leaf_hi.ptr;   // (node 0, or the only leaf)
  float area = 0.0f;
  if (fit && !hip_ok(launch_refit_fit(st, n4), "k_refit_fit", err)) return false;
  if (write && !hip_ok(launch_refit_grid(st, root_lo, root_hi, d_refit_grid_.ptr), "k_grid_params", err)) return false;
  if (fit) {
    if (!hip_ok(hipMemsetAsync(d_refit_area_.ptr, 0, sizeof(float), st), "clear", err) ||
        !hip_ok(launch_refit_quantise(st, n4, d_refit_grid_.ptr, write, d_refit_area_.ptr), "k_refit_quantise", err))
      return false;
    if (t.n_nodes8 && write && (!hip_ok(launch_refit_fit(st, n8), "k_refit_fit", err) || !hip_ok(launch_refit_quantise(st, n8, d_refit_grid_.ptr, true, nullptr), "k_refit_quantise", err)))
      return false;
    if (!hip_ok(hipMemcpyAsync(&area, d_refit_area_.ptr, sizeof(float), hipMemcpyDeviceToHost, st), "read box area", err)) return false;
  }
  out.grid = BvhGrid{};
  if ((write && !hip_ok(hipMemcpyAsync(&out.grid, d_refit_grid_.ptr, sizeof(BvhGrid), hipMemcpyDeviceToHost, st), "read grid", err)) ||
      !hip_ok(hipMemcpyAsync(&out.lo, root_lo, sizeof(float4), hipMemcpyDeviceToHost, st), "read root box", err) ||
      !hip_ok(hipMemcpyAsync(&out.hi, root_hi, sizeof(float4), hipMemcpyDeviceToHost, st), "read root box", err) || !hip_ok(hipStreamSynchronize(st), "refit", err))
    return false;
  p.area = fit ? area : 2.0f * ((out.hi.x - out.lo.x) * (out.hi.y - out.lo.y) + (out.hi.y - out.lo.y) * (out.hi.z - out.lo.z) + (out.hi.z - out.lo.z) * (out.hi.x - out.lo.x));
  return true;
}

bool Accel::prepare_refit(const Sources& s, Error& err) {
  if (!plans_.empty()) return true;
  hipStream_t st = s.stream;
  if (!d_refit_grid_.ptr && (!hip_ok(d_refit_grid_.alloc(1), "alloc", err) || !hip_ok(d_refit_area_.alloc(1), "alloc", err))) return false;
  std::vector<RefitPlan> plans(two_level_ ? tl_meshes_.size() : 1);
  if (two_level_) {
    // what the meshes' builds had: a pseudo-instance each, the identity transform, its flag
    std::vector<RTInstance> pseudo;
    tl_vertex_span_.clear();
    for (const TlMesh& m : tl_meshes_) {
      pseudo.push_back(RTInstance{m.index_offset, m.index_count, 0u, 0u});
      std::pair<uint32_t, uint32_t> span(0xFFFFFFFFu, 0u);
      for (uint32_t k = 0; k < m.index_count; ++k) {
        const uint32_t v = s.data.indices[m.index_offset + k];
        span.first = std::min(span.first, v);
        span.second = std::max(span.second, v);
      }
      tl_vertex_span_.push_back(span);
    }
    TransformPair ident{};
    for (int k = 0; k < 4; ++k) ident.o2w[5 * k] = ident.w2o[5 * k] = 1.0f;
    const uint32_t one = 1u;
    if (!hip_ok(d_tl_pseudo_.upload(pseudo.data(), pseudo.size(), st), "upload", err) || !hip_ok(d_tl_ident_.upload(&ident, 1, st), "upload", err) ||
        !hip_ok(d_tl_one_.upload(&one, 1, st), "upload", err) || !hip_ok(hipStreamSynchronize(st), "upload", err))
      return false;
  }
  for (size_t m = 0; m < plans.size(); ++m) {
    const RefitTarget t = refit_target(s, m);
    const size_t quads_end = !two_level_ ? d_quads_.count : (m + 1 < plans.size() ? h_mesh_ranges[m + 1].quad_base : d_quads_.count - 1);
    const uint32_t n_leaves = (uint32_t)(quads_end - (two_level_ ? h_mesh_ranges[m].quad_base : 0u));
    if (!make_plan(st, t, n_leaves, plans[m], err)) return false;
    // the figure of the structure as the builder left it: the same passes over the vertices it was built from, nothing written but what is there
    RefitResult r;
    if (n_leaves && !refit(st, s, t, plans[m], false, r, err)) return false;
    plans[m].area_built = plans[m].area;
  }
  plans_ = std::move(plans);
  return true;
}

bool Accel::update_geometry(const Sources& s, int mode, uint32_t first, uint32_t count, StreamTimer& timer, Error& err) {
  hipStream_t st = s.stream;
  const Geometry& g = s.geometry;
  uint32_t touched = 0;
  if (mode == GLZ_GEOMETRY_REBUILD) {
    if (!(two_level_ ? build_two_level(s, err) : build_bvh(s, err)) || !hip_ok(hipStreamSynchronize(st), "update_vertices", err)) return false;
    timer.stop(st);
    for (const TlMesh& m : tl_meshes_) touched += m.index_count >= 3u ? 1u : 0u;
    if (!two_level_) touched = 1;
  } else {
    if (!prepare_refit(s, err)) return false;   // (Scene::update_vertices has called it before the vertices changed: nothing left to do)
    if (!two_level_ && plans_[0].n_leaves == 0) {   // a scene without triangles has nothing to refit
      timer.stop(st);
    } else if (!two_level_) {
      RefitResult r;
      if (!refit(st, s, refit_target(s, 0), plans_[0], true, r, err)) return false;
      grid_ = r.grid;
      for (int k = 0; k < 3; ++k) {
        info_.bounds_min[k] = (&r.lo.x)[k];
        info_.bounds_max[k] = (&r.hi.x)[k];
        info_.bvh_grid_lo[k] = r.grid.lo[k];
        info_.bvh_grid_cell[k] = r.grid.cell[k];
      }
      // what the build derives from the nodes and the triangle records, again and unchanged
      if (!hip_ok(launch_top_table(st, d_nodes_.ptr, (uint32_t)d_nodes_.count, d_top_.ptr), "k_top_table", err) ||
          !hip_ok(launch_shade_records(st, n_shade_slots_, d_tris_.ptr, g.instances.ptr, g.indices.ptr, g.vertices.ptr, g.derivatives.ptr, d_xf_identity_.ptr,
                                       d_shade_tris_.ptr), "k_shade_records", err) ||
          !hip_ok(hipStreamSynchronize(st), "shading records", err) || !build_alpha_records(s, err))
        return false;
      timer.stop(st);
      touched = 1;
    } else {
      for (size_t m = 0; m < plans_.size(); ++m) {
        const uint32_t n = tl_meshes_[m].index_count / 3u;
        const std::pair<uint32_t, uint32_t>& span = tl_vertex_span_[m];
        if (n == 0 || span.second < first || span.first >= (uint64_t)first + count) continue;   // (conservative: a mesh may skip vertices inside its span)
        RefitResult r;
        if (!refit(st, s, refit_target(s, m), plans_[m], true, r, err)) return false;
        tl_meshes_[m].grid = r.grid;
        for (int k = 0; k < 3; ++k) {
          tl_meshes_[m].lo[k] = (&r.lo.x)[k];
          tl_meshes_[m].hi[k] = (&r.hi.x)[k];
        }
        const uint32_t tri_base = h_mesh_ranges[m].tri_base;
        if (!hip_ok(launch_shade_records(st, n, d_tris_.ptr + tri_base, d_tl_pseudo_.ptr + m, g.indices.ptr, g.vertices.ptr, g.derivatives.ptr, d_tl_one_.ptr,
                                         d_shade_tris_.ptr + 8 * (size_t)tri_base), "k_shade_records", err))
          return false;
        ++touched;
      }
      tl_points_ready_ = false;   // the cached mesh points and boxes are those of the old vertices
      if (!rebuild(s, err)) return false;   // the top level over the instance boxes of the new meshes
      timer.stop(st);
    }
  }
  update_.mode = (uint32_t)mode;
  update_.meshes_touched = touched;
  update_.update_ms = info_.build_ms = timer.ms();
  update_valid_ = true;
  return true;
}

bool Accel::geometry_update(const Sources& s, glz_geometry_update_info& out, Error& err) {
  if (!update_valid_) return err.fail(GLZ_E_ARG, "geometry_update_info: no update_vertices on this scene yet");
  if (!prepare_refit(s, err)) return false;   // (after a rebuild: the figures of the new structure, and the plan the next refit needs)
  out = update_;
  out.box_area = out.box_area_built = 0.0f;
  for (const RefitPlan& p : plans_) {
    out.box_area += p.area;
    out.box_area_built += p.area_built;
  }
  return true;
}

}  // namespace glz
