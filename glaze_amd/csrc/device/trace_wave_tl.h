// The wave-persistent tracer of two-level (instanced) scenes.
#pragma once
#include "device/trace_wave.h"

namespace glz {
using namespace dev;

// ---------------------------------------------------------------------------------------------
// Two-level traversal (instanced scenes, DeviceScene::two_level; types.h TlasInstance): the same wave-persistent rounds over a
// top level whose leaves are instances and, inside an instance, the mesh's object-space hierarchy.
//   * Entering an instance (a top-level leaf, handled in the leaf phase) pushes an exit marker, takes the ray into object space
//     ONLY to re-derive the grid-space ray of the mesh's own quantisation grid -- with every box widened by the instance's slack,
//     folded into the slab test's addends -- and continues at the mesh's root.  Popping the marker re-derives the top-level
//     grid-space ray from the world ray, which never leaves its registers.
//   * A mesh leaf transforms its one or two OBJECT triangles to world space with the instance's matrix, operation for
//     operation what k_world_tris does for the flattened build, and runs the same world-space Moeller-Trumbore test: hits
//     (t, u, v, tie-break by world triangle id) are bit-identical to the flattened twin of the scene, whatever the hierarchy.
// (Tail work sharing of TOP-level entries -- an idle lane takes the oldest top-level entry below a busy lane's exit marker, with the
// world ray through __shfl and the top-level grid ray from the donor's LDS column, and enters instances on its own -- was built and
// measured: bit-identical, and slower everywhere, forest x 200 0.820 -> 0.864 ms per launch, a 1/8 share 0.160 -> 0.180; once per
// round instead of per node iteration 0.856 / 0.174.  A stolen top-level subtree costs its helper instance entries that the owner,
// with the bound of the hit it finds first, mostly never makes.)
// Simpler than trace_wave on purpose (no tail work sharing; the staged top is built in and off, kTlLdsTop): instanced scenes are about memory -- O(meshes + instances) instead of
// O(instances x triangles) -- and must not put the tuned flattened path at risk.
// ---------------------------------------------------------------------------------------------
constexpr int kExitInstance = 0x7FFFFFFD;   // stack marker: the entries below belong to the top level
// refill / leaf-phase thresholds of the two-level tracer (lanes): defaults = the flattened tracer's
// (Leaf quorum of this tracer, GLZ_TL_LEAF_QUORUM in device/tuning.h: 8 / 16 / 24 / 32 / 40 / 48 lanes -> 0.993 / 0.889 / 0.844 / 0.825 / 0.822 / 0.835 ms
// per launch (forest x 200): a leaf visit here is an instance entry or a triangle taken to world space, dearer than the flattened tracer's.
// The top level's first nodes from a per-block LDS copy, as in the flattened tracer: 0.823 -> 0.833 ms -- built in, off.)
constexpr bool kTlLdsTop = false;

template <bool ANY, bool COUNT, class Source, class Sink>
__device__ __forceinline__ void trace_wave_tl(const DeviceScene& S, Source& src, Sink& sink, int* __restrict__ lds_col, int* aux, int* link_scratch, float* __restrict__ top_ray, LdsNodePtr top_lds,
                                              uint32_t* __restrict__ spill, uint32_t spill_depth, uint32_t total, uint32_t wave, uint32_t n_waves, TraceTally& tally) {
  constexpr uint32_t kNone = 0xFFFFFFFFu;
  wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)wave);   // (uniform, and said so: see trace_wave)
  n_waves = (uint32_t)__builtin_amdgcn_readfirstlane((int)n_waves);
  total = (uint32_t)__builtin_amdgcn_readfirstlane((int)total);
  const BvhNode4* __restrict__ nodes = S.bvh_nodes;        // top-level nodes first, the meshes' after them (TlasInstance::node_base)
  const TlasInstance* __restrict__ instances = S.tlas_instances;
  const int lane = threadIdx.x & 63;
  const unsigned long long lanes_below = (1ull << lane) - 1ull;
  uint32_t seq = 0;
  const RaySequence rays(wave, n_waves, total);
  bool exhausted = rays.ray_at(0u) >= total;
  bool open = false;
  int cur = kRayDone;
  uint32_t ray = 0, nbase = 0, cur_inst = kNone;
  vec3 o = mk3(0.0f, 0.0f, 0.0f), d = mk3(0.0f, 0.0f, 1.0f);                                  // the WORLD ray, always
  vec3 ig = mk3(0.0f, 0.0f, 0.0f), cgn = mk3(0.0f, 0.0f, 0.0f), cgf = mk3(0.0f, 0.0f, 0.0f);    // grid-space ray of the level the lane is in
  SlabSel sel{kSlabSelLo, kSlabSelLo, kSlabSelLo};
  float tmin = 0.0f, tmax = 0.0f;
  HitRecord best{0.0f, 0.0f, 0.0f, kNone, 0u, kNone};
  Stack st{lds_col, spill, spill_depth, 0};
  // grid-space ray for grid g from a ray (oo, dd) given in that grid's space; boxes widened by `slack` (a length in that space)
  // plus `cells` cells on every side
  auto set_grid_ray = [&](const float* glo, const float* gcell, const float* ginv, vec3 oo, vec3 dd, float slack, float cells) {
    const vec3 og = mk3((oo.x - glo[0]) * ginv[0], (oo.y - glo[1]) * ginv[1], (oo.z - glo[2]) * ginv[2]);
    const vec3 id = mk3(grid_inv_dir(dd.x), grid_inv_dir(dd.y), grid_inv_dir(dd.z));
    ig = mk3(id.x * gcell[0], id.y * gcell[1], id.z * gcell[2]);
    const vec3 cg = mk3(grid_addend(og.x, ig.x), grid_addend(og.y, ig.y), grid_addend(og.z, ig.z));
    // The pad as a LENGTH of that space (slack + `cells` cells) over the direction, not as a number of cells: across the thin side of a
    // flat mesh a cell is 1e-13 of a unit, and a pad counted in cells (it was, capped at twice the grid's span) is then far less than the
    // rounding of the transformed ray it stands for -- coplanar meshes lost near ties, thin ones hits (tools/gpu_fuzz_parity.py).
    const vec3 w = mk3((slack + cells * gcell[0]) * fabsf(id.x), (slack + cells * gcell[1]) * fabsf(id.y), (slack + cells * gcell[2]) * fabsf(id.z));
    cgn = cg - w;
    cgf = cg + w;
    sel = SlabSel{slab_sel(ig.x), slab_sel(ig.y), slab_sel(ig.z)};
  };
#ifdef GLZ_WAVE_TIMES
  unsigned long long tl_rays = 0, tl_top = 0, tl_mesh = 0, tl_enter = 0, tl_tris = 0, tl_niter = 0, tl_liter = 0;
#endif
  // The top level's grid-space ray is derived once per ray and parked in the lane's LDS column top_ray[k * kBlock] (k = 0..8: ig, cgn,
  // cgf): leaving an instance reloads it instead of re-deriving it from the world ray (three correctly rounded divisions).
  auto to_top_level = [&](bool fresh) {
    cur_inst = kNone;
    nbase = 0u;
    if (fresh) {
      set_grid_ray(S.bvh_grid.lo, S.bvh_grid.cell, S.bvh_grid.inv_cell, o, d, 0.0f, 0.0f);
      top_ray[0] = ig.x; top_ray[kBlock] = ig.y; top_ray[2 * kBlock] = ig.z;
      top_ray[3 * kBlock] = cgn.x; top_ray[4 * kBlock] = cgn.y; top_ray[5 * kBlock] = cgn.z;
      top_ray[6 * kBlock] = cgf.x; top_ray[7 * kBlock] = cgf.y; top_ray[8 * kBlock] = cgf.z;
    } else {
      ig = mk3(top_ray[0], top_ray[kBlock], top_ray[2 * kBlock]);
      cgn = mk3(top_ray[3 * kBlock], top_ray[4 * kBlock], top_ray[5 * kBlock]);
      cgf = mk3(top_ray[6 * kBlock], top_ray[7 * kBlock], top_ray[8 * kBlock]);
      sel = SlabSel{slab_sel(ig.x), slab_sel(ig.y), slab_sel(ig.z)};
    }
  };
  auto pop_next = [&]() -> int {
    for (;;) {
      if (st.sp == 0) return kRayDone;
      const int v = st.pop();
      if (v != kExitInstance) return v;
      to_top_level(false);
    }
  };
  const uint32_t prio_gen = (blockIdx.x * 4u) / gridDim.x;   // (four blocks per CU here)
  uint32_t prio_round = 0;
  for (;;) {
    if (rays.own_full >= 128u) rotate_priority(prio_gen + prio_round++);
    // ---- refill ----
    const unsigned long long idle = __ballot(!open);
    const int n_idle = __popcll(idle);
    if (!exhausted && n_idle >= kTlRefill) {
      const uint32_t next_ray = rays.ray_at(seq + (uint32_t)__popcll(idle & lanes_below));
      if (!open && next_ray < total) {
        if (src.load(next_ray, o, d, tmin, tmax)) {
          ray = next_ray;
          best = HitRecord{tmax, 0.0f, 0.0f, kNone, 0u, kNone};
          if (COUNT) tally.rays += 1;
          if (S.n_world_tris == 0 || !ray_is_finite(o, d)) {
            sink.store(ray, best);
          } else {
            st.sp = 0;
            to_top_level(true);
            cur = kTlLdsTop ? kBvhTopFlag : 0;   // the top level's root (slot 0 of the staged table)
            open = true;
#ifdef GLZ_WAVE_TIMES
            tl_rays += 1;
#endif
          }
        }
      }
      seq += (uint32_t)n_idle;
      exhausted = rays.ray_at(seq) >= total;
    }
    if (__ballot(open) == 0ull) {
      if (exhausted) break;
      continue;
    }
    // ---- inner-node phase (either level) ----
    for (;;) {
      const bool at_node = cur >= 0 && cur < kExitInstance;
      if (__ballot(at_node) == 0ull) break;
#ifdef GLZ_WAVE_TIMES
      if (lane == 0) tl_niter += 1;
      if (at_node) { if (cur_inst == kNone) tl_top += 1; else tl_mesh += 1; }
#endif
      if (at_node) {
        if (COUNT) tally.nodes += 1;   // node visits of either level
        // the top level's first kBvhTopNodes nodes come out of the block's LDS copy (`cur` = kBvhTopFlag | slot), like the flattened tracer's
        u32x4 w0, w1, w2, w3;
        if (kTlLdsTop && (cur & kBvhTopFlag)) {
          LdsNodePtr np = top_lds + 4 * (cur & 0xFFFF);
          w0 = np[0]; w1 = np[1]; w2 = np[2]; w3 = np[3];
        } else {
          const u32x4* np = reinterpret_cast<const u32x4*>(record_at(nodes, nbase + (uint32_t)cur));   // (base plus a 32-bit byte offset: trace_wave.h record_at)
          w0 = np[0]; w1 = np[1]; w2 = np[2]; w3 = np[3];
        }
        uint32_t k0 = box_key(w0.x, w0.y, w0.z, w3.x, 0u, sel, ig, cgn, cgf, tmin, best.t), k1 = box_key(w0.w, w1.x, w1.y, w3.y, kKeyChild, sel, ig, cgn, cgf, tmin, best.t);
        uint32_t k2 = box_key(w1.z, w1.w, w2.x, w3.z, 2u * kKeyChild, sel, ig, cgn, cgf, tmin, best.t), k3 = box_key(w2.y, w2.z, w2.w, w3.w, 3u * kKeyChild, sel, ig, cgn, cgf, tmin, best.t);
        sort4(k0, k1, k2, k3);   // (device/sort4.h; equal keys are miss markers, which nothing tells apart: see trace_wave)
        int* links = link_scratch + lane;
        links[0] = (int)w3.x; links[64] = (int)w3.y; links[128] = (int)w3.z; links[192] = (int)w3.w;
        const uint32_t link_base = (uint32_t)(uintptr_t)(LdsIntPtr)links;   // the wave's area is 1 KB aligned: bits 8..9 are the child's
        const int l0 = sorted_link(link_base, k0), l1 = sorted_link(link_base, k1), l2 = sorted_link(link_base, k2), l3 = sorted_link(link_base, k3);
        if (k0 == 0xFFFFFFFFu) {
          cur = pop_next();
        } else {
          if (__ballot(st.sp + 3 > kLdsStack) == 0ull) {   // wave-uniform: every lane stays inside the LDS part of its stack (no spill branches)
            if (k3 != 0xFFFFFFFFu) { st.lds[st.sp * kBlock] = l3; ++st.sp; }
            if (k2 != 0xFFFFFFFFu) { st.lds[st.sp * kBlock] = l2; ++st.sp; }
            if (k1 != 0xFFFFFFFFu) { st.lds[st.sp * kBlock] = l1; ++st.sp; }
          } else {
            if (k3 != 0xFFFFFFFFu) st.push(l3);
            if (k2 != 0xFFFFFFFFu) st.push(l2);
            if (k1 != 0xFFFFFFFFu) st.push(l1);
          }
          cur = l0;
        }
      }
      // (Instance entries and triangle tests with a quorum each -- 8 / 16 / 24 lanes for entries, 24 / 32 for triangles -- so that neither kind of
      // leaf work runs for a handful of lanes: forest x 200 0.803 -> 0.816 ... 0.838 ms per launch, x 2 000 1.082 -> 1.106 ... 1.129: slower.)
      if (__popcll(__ballot(cur < 0)) >= GLZ_TL_LEAF_QUORUM) break;
    }
    // ---- leaf phase: an instance to enter (top level) or triangles to test (inside an instance) ----
    if (cur < 0) {
      if (cur_inst == kNone) {
        cur_inst = (uint32_t)~cur;
        const TlasInstance* ti = record_at(instances, cur_inst);
        const float4* q = reinterpret_cast<const float4*>(ti->w2o);
        const float4 r0 = q[0], r1 = q[1], r2 = q[2];
        // object-space ray (a point and a vector through the 3 x 4 matrix): only the box tests see it
        const vec3 oo = mk3(((r0.x * o.x + r0.y * o.y) + r0.z * o.z) + r0.w, ((r1.x * o.x + r1.y * o.y) + r1.z * o.z) + r1.w, ((r2.x * o.x + r2.y * o.y) + r2.z * o.z) + r2.w);
        const vec3 dd = mk3((r0.x * d.x + r0.y * d.y) + r0.z * d.z, (r1.x * d.x + r1.y * d.y) + r1.z * d.z, (r2.x * d.x + r2.y * d.y) + r2.z * d.z);
        st.push(kExitInstance);
        nbase = ti->node_base;
        // The slack the build computed covers ray origins inside the scene's bounds; the rounding of oo grows with |o|, wherever the
        // ray starts (a camera far outside a small instanced scene): 32 eps |W2O|_inf |o|_1 on top, in object units like the rest.
        const float slack = ti->slack + (3.8146973e-6f * ti->w2o_norm) * ((fabsf(o.x) + fabsf(o.y)) + fabsf(o.z));
        set_grid_ray(ti->grid.lo, ti->grid.cell, ti->grid.inv_cell, oo, dd, slack, 1.0f);
        cur = 0;   // the mesh's root
      } else {
        const TlasInstance* ti = record_at(instances, cur_inst);
        // The mesh's leaf record (types.h BvhQuad; its hierarchy was built over the mesh under the identity transform, so the
        // vertices are the object-space ones): one 64-byte line for one triangle or two.  The world triangles are exactly what
        // k_world_tris builds -- points through o2w -- four of them for a pair instead of six.
        const float4* qp = reinterpret_cast<const float4*>(record_at(S.bvh_quads, ti->quad_base + (uint32_t)~cur));
        const float4 r0 = qp[0], r1 = qp[1], r2 = qp[2], r3 = qp[3];
        const uint32_t id0 = __float_as_uint(r0.w), qflags = __float_as_uint(r2.w), slot0 = ti->tri_base + __float_as_uint(r3.w);
        const bool pair = (qflags & kTriHasPartner) != 0u;
        if (COUNT) tally.tris += pair ? 2 : 1;
        const vec3 w0 = xform_point(ti->o2w, mk3(r0.x, r0.y, r0.z)), w1 = xform_point(ti->o2w, mk3(r1.x, r1.y, r1.z));
        const vec3 w2 = xform_point(ti->o2w, mk3(r2.x, r2.y, r2.z)), w3 = xform_point(ti->o2w, mk3(r3.x, r3.y, r3.z));
        const RayShear rs = ray_shear(d);
        const QuadHit qh = ray_quad(rs, make_float4(w0.x, w0.y, w0.z, 0.0f), make_float4(w1.x, w1.y, w1.z, 0.0f), make_float4(w2.x, w2.y, w2.z, 0.0f),
                                    make_float4(w3.x, w3.y, w3.z, 0.0f), pair, o, tmin);
        const uint32_t swapped = (qflags & kQuadSwapped) ? 1u : 0u;
        bool finished = false;
#pragma nounroll
        for (uint32_t which = 0; which < 2u; ++which) {   // the leaf's first triangle, then its partner (the order the 48-byte records were walked in)
          const bool is_b = (which ^ swapped) != 0u;
          const float t = is_b ? qh.t[1] : qh.t[0], u = is_b ? qh.u[1] : qh.u[0], v = is_b ? qh.v[1] : qh.v[0];
          if ((is_b ? qh.ok[1] : qh.ok[0]) && t < tmax) {
            const uint32_t world_id = ti->world_base + id0 + which, slot = slot0 + which;
            const bool better = best.leaf == kNone ? true : (t < best.t || (t == best.t && world_id < best.world_id));
            if (better && (ti->non_opaque == 0u || alpha_test_instance(S, slot, ti->instance, u, v))) {
              best = HitRecord{t, u, v, slot, ti->instance, world_id};
              finished = ANY;
            }
          }
        }
        cur = finished ? kRayDone : pop_next();
      }
    }
    // ---- retire ----
    if (open && cur == kRayDone) {
      if (COUNT) tally.hits += best.leaf != kNone;
      sink.store(ray, best);
      open = false;
    }
  }
  __builtin_amdgcn_s_setprio(0);
#ifdef GLZ_WAVE_TIMES
  if (!ANY) {
    atomicAdd(&g_tl_stats[0], tl_rays); atomicAdd(&g_tl_stats[1], tl_top); atomicAdd(&g_tl_stats[2], tl_mesh); atomicAdd(&g_tl_stats[3], tl_enter);
    atomicAdd(&g_tl_stats[4], tl_tris); atomicAdd(&g_tl_stats[5], tl_niter); atomicAdd(&g_tl_stats[6], tl_liter);
  }
#endif
}
}  // namespace glz
