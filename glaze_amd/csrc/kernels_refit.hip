// Refit kernels for gfx950: new vertices under a hierarchy that keeps its topology (Accel::update_geometry).  The leaf records and leaf
// boxes are recomputed by the build's own rules (build_common.h), the wide nodes' float boxes are fitted level by level from the
// leaves up, the grid is re-derived from the root box as the build derives it, and every child box is quantised again.  Like the
// build's bottom-up passes (kernels_build.hip, above k_node_depth) the kernel boundary is the only synchronisation.
#include <hip/hip_runtime.h>

#include "build_common.h"
#include "device/math.h"
#include "device/types.h"
#include "kernels.h"

namespace glz {
using namespace dev;

// One thread per leaf record: the record names its instance, its first primitive and its first triangle slot, which is all that is
// needed to write the leaf again -- its one or two BvhTri, the record's corners and the leaf's box.  For a mesh of a two-level scene
// `instances` is the mesh's pseudo-instance and `transforms` the identity, as in its build.
__global__ void __launch_bounds__(256) k_refit_leaves(const float4* __restrict__ vertices, const uint32_t* __restrict__ indices,
                                                      const RTInstance* __restrict__ instances, const TransformPair* __restrict__ transforms,
                                                      uint32_t n_leaves, BvhQuad* __restrict__ quads, BvhTri* __restrict__ tris,
                                                      float4* __restrict__ leaf_lo, float4* __restrict__ leaf_hi) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n_leaves) return;
  BvhQuad q = quads[j];
  const RTInstance in = instances[q.instance];
  const uint32_t prim = q.prim_flags & kQuadPrimMask;
  const bool paired = (q.prim_flags & kTriHasPartner) != 0, swapped = (q.prim_flags & kQuadSwapped) != 0;
  const uint32_t* ix = indices + in.index_offset + 3 * prim;
  const float* M = transforms[in.transform_id].o2w;
  vec3 v[3];
  float l[3], h[3];
  world_triangle(vertices, ix, M, v);
  BvhTri t;
  set_tri_vertices(t, v);
  t.world_id = q.world_id;
  t.instance = q.instance;
  t.prim_flags = q.prim_flags & ~kQuadSwapped;
  padded_tri_box(v, l, h);
  float4 lo = make_float4(l[0], l[1], l[2], 0.0f), hi = make_float4(h[0], h[1], h[2], 0.0f);
  BvhTri b;
  if (paired) {   // the next primitive of the same instance, in the next slot
    world_triangle(vertices, ix + 3, M, v);
    set_tri_vertices(b, v);
    b.world_id = q.world_id + 1u;
    b.instance = q.instance;
    b.prim_flags = (prim + 1u) | (q.prim_flags & kTriNonOpaque);
    padded_tri_box(v, l, h);
    lo = union_lo(lo, make_float4(l[0], l[1], l[2], 0.0f));
    hi = union_hi(hi, make_float4(h[0], h[1], h[2], 0.0f));
    tris[q.slot + 1u] = b;
  }
  tris[q.slot] = t;
  quad_corners(q, t, b, paired && !swapped, paired && swapped);
  quads[j] = q;
  leaf_lo[j] = lo;
  leaf_hi[j] = hi;
}

// the float box of child k of a W-wide node: a leaf's (link < 0: ~leaf number), a node's, or for an empty slot the union's neutral element
__device__ __forceinline__ void child_box(int link, const float4* __restrict__ leaf_lo, const float4* __restrict__ leaf_hi,
                                          const float4* node_lo, const float4* node_hi, float4& lo, float4& hi) {
  lo = make_float4(INFINITY, INFINITY, INFINITY, 0.0f);
  hi = make_float4(-INFINITY, -INFINITY, -INFINITY, 0.0f);
  if (link == kBvhEmptyChild) return;
  lo = link < 0 ? leaf_lo[~link] : node_lo[link];
  hi = link < 0 ? leaf_hi[~link] : node_hi[link];
}

// One level of the fit: W lanes per node, lane k fetches child k's 32-byte box (the children of a node are scattered: W fetches in
// flight per node instead of W in a row), then the W lanes fold their boxes.  min / max order -0 below +0 on this hardware, so the
// fold gives the bits of the build's binary unions whatever its order.  The nodes of a level are `order[first .. first + count)`;
// their inner children lie on lower levels, finished by the launches before.
template <int W>
__global__ void __launch_bounds__(256) k_refit_fit(const uint32_t* __restrict__ nodes /* W-wide, 4 W words each */, const uint32_t* __restrict__ order,
                                                   uint32_t first, uint32_t count, const float4* __restrict__ leaf_lo, const float4* __restrict__ leaf_hi,
                                                   float4* node_lo, float4* node_hi) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t i = t / W, k = t % W;
  const bool live = i < count;
  const uint32_t node = live ? order[first + i] : 0u;
  const int link = live ? (int)nodes[(size_t)node * (4 * W) + 3 * W + k] : kBvhEmptyChild;
  float4 lo, hi;
  child_box(link, leaf_lo, leaf_hi, node_lo, node_hi, lo, hi);
#pragma unroll
  for (int off = 1; off < W; off <<= 1) {   // (W divides the wave: the partners of a lane belong to the same node)
    const float4 l2 = make_float4(__shfl_xor(lo.x, off), __shfl_xor(lo.y, off), __shfl_xor(lo.z, off), 0.0f);
    const float4 h2 = make_float4(__shfl_xor(hi.x, off), __shfl_xor(hi.y, off), __shfl_xor(hi.z, off), 0.0f);
    lo = union_lo(lo, l2);
    hi = union_hi(hi, h2);
  }
  if (live && k == 0) {
    node_lo[node] = lo;
    node_hi[node] = hi;
  }
}

// Every child box on the grid again: one lane per child slot writes its three words; links stay, and so do the words of an empty slot.
// area (may be null): adds the surface areas of the children's float boxes, one atomic per wave (reported only: the order is not fixed).
// write = 0: the sum alone.
template <int W>
__global__ void __launch_bounds__(256) k_refit_quantise(uint32_t* __restrict__ nodes, uint32_t n_nodes, const float4* __restrict__ leaf_lo,
                                                        const float4* __restrict__ leaf_hi, const float4* __restrict__ node_lo,
                                                        const float4* __restrict__ node_hi, const BvhGrid* __restrict__ grid, uint32_t write,
                                                        float* __restrict__ area) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t node = t / W, k = t % W;
  const int link = node < n_nodes ? (int)nodes[(size_t)node * (4 * W) + 3 * W + k] : kBvhEmptyChild;
  float a = 0.0f;
  if (link != kBvhEmptyChild) {
    float4 lo, hi;
    child_box(link, leaf_lo, leaf_hi, node_lo, node_hi, lo, hi);
    if (write) {
      const BvhGrid g = *grid;
      float gm[3];
      grid_margin(g, gm);
      quant_box(lo, hi, g, gm, nodes + (size_t)node * (4 * W) + 3 * k);
    }
    a = box_area(lo, hi);
  }
  if (area) {
    for (int off = 32; off > 0; off >>= 1) a += __shfl_xor(a, off);
    if ((threadIdx.x & 63) == 0) atomicAdd(area, a);
  }
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
hipError_t launch_refit_leaves(hipStream_t st, const float4* vertices, const uint32_t* indices, const RTInstance* instances, const TransformPair* transforms,
                               uint32_t n_leaves, BvhQuad* quads, BvhTri* tris, float4* leaf_lo, float4* leaf_hi) {
  if (n_leaves == 0) return hipSuccess;
  return launch(k_refit_leaves, dim3((n_leaves + 255) / 256), dim3(256), st, vertices, indices, instances, transforms, n_leaves, quads, tris, leaf_lo, leaf_hi);
}

template <int W>
static hipError_t fit_levels(hipStream_t st, const RefitNodes& n) {
  for (size_t level = 0; level + 1 < n.level_first.size(); ++level) {   // level 0: the nodes over leaves alone, the deepest in the tree
    const uint32_t first = n.level_first[level], count = n.level_first[level + 1] - first;
    if (count == 0) continue;
    GLZ_TRY(launch(k_refit_fit<W>, dim3((uint32_t)(((size_t)count * W + 255) / 256)), dim3(256), st, static_cast<const uint32_t*>(n.nodes), n.order, first, count,
                   n.leaf_lo, n.leaf_hi, n.node_lo, n.node_hi));
  }
  return hipSuccess;
}
hipError_t launch_refit_fit(hipStream_t st, const RefitNodes& n) { return n.width == 8 ? fit_levels<8>(st, n) : fit_levels<4>(st, n); }

hipError_t launch_refit_grid(hipStream_t st, const float4* root_lo, const float4* root_hi, BvhGrid* grid) {
  return launch_grid_params(st, root_lo, root_hi, grid);   // the build's own k_grid_params
}

hipError_t launch_refit_quantise(hipStream_t st, const RefitNodes& n, const BvhGrid* grid, bool write, float* area) {
  if (n.n_nodes == 0) return hipSuccess;
  const dim3 grd((uint32_t)(((size_t)n.n_nodes * n.width + 255) / 256)), blk(256);
  uint32_t* nodes = static_cast<uint32_t*>(n.nodes);
  if (n.width == 8) return launch(k_refit_quantise<8>, grd, blk, st, nodes, n.n_nodes, n.leaf_lo, n.leaf_hi, n.node_lo, n.node_hi, grid, write ? 1u : 0u, area);
  return launch(k_refit_quantise<4>, grd, blk, st, nodes, n.n_nodes, n.leaf_lo, n.leaf_hi, n.node_lo, n.node_hi, grid, write ? 1u : 0u, area);
}

}  // namespace glz
