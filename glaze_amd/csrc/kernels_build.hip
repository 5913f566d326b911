// Scene-build kernels for gfx950: instance flattening, leaves in Morton order (Morton codes -> bitonic sort), the LBVH
// (Karras hierarchy) and PLOC builders, and what follows any builder (bottom-up fit -> depth-first layout -> wide collapse): the
// hierarchy that replaces the driver's BLAS/TLAS build (lib/src/vulkan/acceleration.rs:89-494).  The binned SAH builder on the
// device is kernels_build_sah.hip; build_hierarchy at the end of this file runs the stages.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "build_common.h"
#include "device/math.h"
#include "device/types.h"
#include "kernels.h"

namespace glz {
using namespace dev;

// ---------------------------------------------------------------------------------------------
// Instance flattening: world triangle w -> (instance, primitive), world-space v0/e1/e2 + AABB.
// Scene bounds are reduced per block in LDS, then one ordered-int atomic per block and axis.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_world_tris(const float4* __restrict__ vertices, const uint32_t* __restrict__ indices,
                                                    const RTInstance* __restrict__ instances, const uint32_t* __restrict__ inst_base,
                                                    uint32_t n_instances, const TransformPair* __restrict__ transforms,
                                                    const RTMaterial* __restrict__ materials, uint32_t n_world,
                                                    BvhTri* __restrict__ tris, float4* __restrict__ box_lo, float4* __restrict__ box_hi,
                                                    int* __restrict__ scene_bounds /* 6 ordered ints: centroid lo xyz, hi xyz */) {
  __shared__ float s_lo[3][256], s_hi[3][256];
  const uint32_t w = blockIdx.x * blockDim.x + threadIdx.x;
  float clo[3] = {INFINITY, INFINITY, INFINITY}, chi[3] = {-INFINITY, -INFINITY, -INFINITY};
  if (w < n_world) {
    // binary search: last instance whose first world triangle is <= w
    uint32_t lo = 0, hi = n_instances - 1;
    while (lo < hi) {
      uint32_t mid = (lo + hi + 1) >> 1;
      if (inst_base[mid] <= w) lo = mid; else hi = mid - 1;
    }
    const uint32_t inst = lo, prim = w - inst_base[inst];
    const RTInstance in = instances[inst];
    const uint32_t* ix = indices + in.index_offset + 3 * prim;
    const float* M = transforms[in.transform_id].o2w;
    vec3 v[3];
    world_triangle(vertices, ix, M, v);
    BvhTri t;
    set_tri_vertices(t, v);
    t.world_id = w;
    t.instance = inst;
    t.prim_flags = prim | (materials[in.material_id].opacity != 0 ? kTriNonOpaque : 0u);   // acceleration.rs:136-141
    tris[w] = t;
    float l[3], h[3];
    padded_tri_box(v, l, h);
#pragma unroll
    for (int k = 0; k < 3; ++k) clo[k] = chi[k] = 0.5f * (l[k] + h[k]);
    box_lo[w] = make_float4(l[0], l[1], l[2], 0.0f);
    box_hi[w] = make_float4(h[0], h[1], h[2], 0.0f);
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) { s_lo[k][threadIdx.x] = clo[k]; s_hi[k][threadIdx.x] = chi[k]; }
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (threadIdx.x < s) {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        s_lo[k][threadIdx.x] = fminf(s_lo[k][threadIdx.x], s_lo[k][threadIdx.x + s]);
        s_hi[k][threadIdx.x] = fmaxf(s_hi[k][threadIdx.x], s_hi[k][threadIdx.x + s]);
      }
    }
    __syncthreads();
  }
  if (threadIdx.x < 3) {
    atomicMin(&scene_bounds[threadIdx.x], float_to_ordered(s_lo[threadIdx.x][0]));
    atomicMax(&scene_bounds[3 + threadIdx.x], float_to_ordered(s_hi[threadIdx.x][0]));
  }
}

// 21 bits per axis interleaved to a 63-bit Morton code
__device__ __forceinline__ uint64_t spread21(uint64_t x) {
  x &= 0x1FFFFFull;
  x = (x | x << 32) & 0x1F00000000FFFFull;
  x = (x | x << 16) & 0x1F0000FF0000FFull;
  x = (x | x << 8) & 0x100F00F00F00F00Full;
  x = (x | x << 4) & 0x10C30C30C30C30C3ull;
  x = (x | x << 2) & 0x1249249249249249ull;
  return x;
}

__global__ void __launch_bounds__(256) k_morton(const float4* __restrict__ box_lo, const float4* __restrict__ box_hi,
                                                const int* __restrict__ scene_bounds, uint32_t n, uint32_t n_padded,
                                                uint64_t* __restrict__ keys, uint32_t* __restrict__ vals) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_padded) return;
  if (i >= n) {   // padding of the power-of-two bitonic network sorts to the end
    keys[i] = ~0ull;
    vals[i] = 0xFFFFFFFFu;
    return;
  }
  float q[3];
  float c[3];
  box_centroid(box_lo[i], box_hi[i], c);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float lo = ordered_to_float(scene_bounds[k]), hi = ordered_to_float(scene_bounds[3 + k]);
    const float ext = hi - lo;
    float t = ext > 0.0f ? (c[k] - lo) / ext : 0.0f;
    t = fminf(fmaxf(t, 0.0f), 1.0f);
    q[k] = fminf(t * 2097152.0f, 2097151.0f);
  }
  keys[i] = (spread21((uint64_t)q[0]) << 2) | (spread21((uint64_t)q[1]) << 1) | spread21((uint64_t)q[2]);
  vals[i] = i;
}

// ---------------------------------------------------------------------------------------------
// Bitonic sort of (key, value) pairs, n a power of two.  Strides >= 1024 run one compare-exchange
// per launch in global memory; all strides below are fused in LDS (2048 pairs per 1024-thread block).
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ bool key_greater(uint64_t ka, uint32_t va, uint64_t kb, uint32_t vb) {
  return ka > kb || (ka == kb && va > vb);
}

__global__ void __launch_bounds__(256) k_bitonic_global(uint64_t* __restrict__ keys, uint32_t* __restrict__ vals, uint32_t n, uint32_t k,
                                                        uint32_t j) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;   // one thread per pair
  if (t >= n / 2) return;
  const uint32_t i = 2 * t - (t & (j - 1));   // index with bit j cleared
  const uint32_t p = i + j;
  const bool up = (i & k) == 0;
  const uint64_t ka = keys[i], kb = keys[p];
  const uint32_t va = vals[i], vb = vals[p];
  if (key_greater(ka, va, kb, vb) == up) {
    keys[i] = kb; keys[p] = ka;
    vals[i] = vb; vals[p] = va;
  }
}

constexpr uint32_t kSortTile = 2048;
__global__ void __launch_bounds__(1024) k_bitonic_lds(uint64_t* __restrict__ keys, uint32_t* __restrict__ vals, uint32_t n, uint32_t k_first,
                                                      uint32_t k_last, uint32_t j_first) {
  // Runs, for k = k_first..k_last (doubling), the strides j = min(j_first or k/2, 1024) .. 1 inside one tile.
  __shared__ uint64_t s_k[kSortTile];
  __shared__ uint32_t s_v[kSortTile];
  const uint32_t base = blockIdx.x * kSortTile;
  for (uint32_t t = threadIdx.x; t < kSortTile; t += blockDim.x) {
    s_k[t] = keys[base + t];
    s_v[t] = vals[base + t];
  }
  __syncthreads();
  for (uint32_t k = k_first; k <= k_last; k <<= 1) {
    uint32_t j = (k == k_first && j_first) ? j_first : k >> 1;
    if (j > kSortTile / 2) j = kSortTile / 2;
    for (; j > 0; j >>= 1) {
      const uint32_t t = threadIdx.x;
      const uint32_t i = 2 * t - (t & (j - 1));
      const uint32_t p = i + j;
      const bool up = ((base + i) & k) == 0;
      const uint64_t ka = s_k[i], kb = s_k[p];
      const uint32_t va = s_v[i], vb = s_v[p];
      if (key_greater(ka, va, kb, vb) == up) {
        s_k[i] = kb; s_k[p] = ka;
        s_v[i] = vb; s_v[p] = va;
      }
      __syncthreads();
    }
  }
  for (uint32_t t = threadIdx.x; t < kSortTile; t += blockDim.x) {
    keys[base + t] = s_k[t];
    vals[base + t] = s_v[t];
  }
}

// ---------------------------------------------------------------------------------------------
// Leaves.  Two triangles of one instance that follow each other in the index buffer, share an edge and have largely the
// same box (the two halves of a quad: what tessellated grids and triangulated quad meshes consist of) form ONE leaf: the
// hierarchy is built over half as many primitives and the tracer tests both triangles in one leaf round.  A leaf's
// triangles are adjacent in bvh_tris (the first one carries kTriHasPartner); leaf links point at the first.
// Pairs start at even primitives first, then at odd ones between triangles that are still single.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_pair_triangles(uint32_t n_world, uint32_t parity, const BvhTri* __restrict__ tris,
                                                        const uint32_t* __restrict__ indices, const RTInstance* __restrict__ instances,
                                                        const float4* __restrict__ box_lo, const float4* __restrict__ box_hi,
                                                        float area_ratio, uint32_t quads_only,
                                                        uint8_t* role /* 0 single, 1 / 5 first of a pair (5: kQuadSwapped order), 2 second of a pair */) {
  const uint32_t w = blockIdx.x * blockDim.x + threadIdx.x;
  if (w + 1 >= n_world) return;
  const BvhTri a = tris[w], b = tris[w + 1];
  const uint32_t prim = a.prim_flags & kTriPrimMask;
  if ((prim & 1u) != parity || a.instance != b.instance) return;
  if (parity == 1u && (role[w] != 0 || role[w + 1] != 0)) return;
  const RTInstance in = instances[a.instance];
  const uint32_t* ia = indices + in.index_offset + 3 * prim;
  const uint32_t* ib = ia + 3;
  int shared = 0;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) shared += ia[i] == ib[j] ? 1 : 0;
  if (shared != 2) return;
  // The vertex order of the second triangle in terms of the first one's corners (3 = its own fourth vertex).  A quad record
  // (types.h BvhQuad) holds A = (q0, q1, q2), B = (q0, q2, q3): the pair fits as it is when the second triangle reads (0, 2, 3), and
  // with the two triangles in the other order when it reads (0, 3, 1) -- then the SECOND one is A = (p0, d, p1) and the first one
  // (p0, p1, p2) = (q0, q2, q3) is B.  Together these are the two ways a quad is cut into a fan from a shared first vertex (all pairs of the
  // atrium, 98 % of mattest.glaze's); other orders stay single triangles, because re-ordering a triangle's vertices would change the
  // rounding of its (t, u, v).
  uint32_t pat = 0;
  for (int j = 0; j < 3; ++j) {
    uint32_t m = 3;
    for (int i = 0; i < 3; ++i) m = ia[i] == ib[j] ? (uint32_t)i : m;
    pat |= m << (4 * j);
  }
  const bool fits = pat == 0x320u, fits_swapped = pat == 0x130u;   // (0, 2, 3) / (0, 3, 1), first entry in the low nibble
  if (quads_only && !fits && !fits_swapped) return;
  const float4 la = box_lo[w], ha = box_hi[w], lb = box_lo[w + 1], hb = box_hi[w + 1];
  const float4 lm = make_float4(fminf(la.x, lb.x), fminf(la.y, lb.y), fminf(la.z, lb.z), 0.0f);
  const float4 hm = make_float4(fmaxf(ha.x, hb.x), fmaxf(ha.y, hb.y), fmaxf(ha.z, hb.z), 0.0f);
  // one box for both must not cost more than it saves: identical boxes give 0.5, two squares side by side 0.83
  if (!(box_area(lm, hm) <= area_ratio * (box_area(la, ha) + box_area(lb, hb)))) return;
  role[w] = (quads_only && fits_swapped) ? 5 : 1;
  role[w + 1] = 2;
}
__global__ void __launch_bounds__(256) k_leaf_flags(uint32_t n_world, const uint8_t* __restrict__ role, unsigned long long* __restrict__ flags) {
  const uint32_t w = blockIdx.x * blockDim.x + threadIdx.x;
  if (w < n_world) flags[w] = role[w] != 2 ? 1ull : 0ull;
}
// leaf l (numbered in world-triangle order) -> its first triangle and its box
__global__ void __launch_bounds__(256) k_leaf_boxes(uint32_t n_world, const uint8_t* __restrict__ role, const unsigned long long* __restrict__ pos,
                                                    const float4* __restrict__ box_lo, const float4* __restrict__ box_hi,
                                                    uint32_t* __restrict__ leaf_first, float4* __restrict__ leaf_lo, float4* __restrict__ leaf_hi) {
  const uint32_t w = blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= n_world || role[w] == 2) return;
  const uint32_t l = (uint32_t)pos[w];
  float4 lo = box_lo[w], hi = box_hi[w];
  if (role[w] & 1) {
    lo = union_lo(lo, box_lo[w + 1]);
    hi = union_hi(hi, box_hi[w + 1]);
  }
  leaf_first[l] = w;
  leaf_lo[l] = lo;
  leaf_hi[l] = hi;
}
// triangles of the leaf at sorted place j (for the prefix sum that gives its first slot in bvh_tris)
__global__ void __launch_bounds__(256) k_leaf_sizes(uint32_t n, const uint32_t* __restrict__ vals, const uint32_t* __restrict__ leaf_first,
                                                    const uint8_t* __restrict__ role, unsigned long long* __restrict__ sizes) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j < n) sizes[j] = (role[leaf_first[vals[j]]] & 1) ? 2ull : 1ull;
}

// gathers triangles and boxes into leaf (sorted) order
__global__ void __launch_bounds__(256) k_gather_leaves(const uint32_t* __restrict__ vals, uint32_t n, const uint32_t* __restrict__ leaf_first,
                                                       const uint8_t* __restrict__ role, const unsigned long long* __restrict__ slot,
                                                       const BvhTri* __restrict__ tris_in, const float4* __restrict__ lo_in,
                                                       const float4* __restrict__ hi_in, BvhTri* __restrict__ tris_out, float4* __restrict__ node_lo,
                                                       float4* __restrict__ node_hi, BvhQuad* __restrict__ quads_out /* null: none */) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const uint32_t leaf = vals[j], first = leaf_first[leaf];
  const uint32_t s = (uint32_t)slot[j];
  BvhTri t = tris_in[first];
  if (role[first] & 1) {
    t.prim_flags |= kTriHasPartner;
    tris_out[s + 1] = tris_in[first + 1];
  }
  tris_out[s] = t;
  if (quads_out) {
    // the leaf's record for the flattened tracer (types.h BvhQuad): A = (q0, q1, q2), B = (q0, q2, q3)
    BvhQuad q;
    q.world_id = t.world_id;
    q.instance = t.instance;
    q.prim_flags = t.prim_flags;
    q.slot = s;
    quad_corners(q, t, tris_in[first + 1], role[first] == 1, role[first] == 5);
    quads_out[j] = q;
  }
  node_lo[(n - 1) + j] = lo_in[leaf];   // leaf j's box lives at slot (n-1)+j, inner node i's at slot i
  node_hi[(n - 1) + j] = hi_in[leaf];
}

// ---------------------------------------------------------------------------------------------
// Karras 2012: one thread per internal node finds its key range and split
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ int common_prefix(const uint64_t* __restrict__ keys, int n, int i, int j) {
  if (j < 0 || j >= n) return -1;
  const uint64_t x = keys[i] ^ keys[j];
  if (x == 0) return 64 + __clz(i ^ j);   // duplicate codes: fall back to the index bits
  return __clzll((long long)x);
}

__global__ void __launch_bounds__(256) k_hierarchy(const uint64_t* __restrict__ keys, int n, int2* __restrict__ children,
                                                   int* __restrict__ parent) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n - 1) return;
  const int d = common_prefix(keys, n, i, i + 1) - common_prefix(keys, n, i, i - 1) >= 0 ? 1 : -1;
  const int dmin = common_prefix(keys, n, i, i - d);
  int lmax = 2;
  while (common_prefix(keys, n, i, i + lmax * d) > dmin) lmax <<= 1;
  int l = 0;
  for (int t = lmax >> 1; t > 0; t >>= 1)
    if (common_prefix(keys, n, i, i + (l + t) * d) > dmin) l += t;
  const int j = i + l * d;
  const int dnode = common_prefix(keys, n, i, j);
  int s = 0;
  for (int t = (l + 1) >> 1;; t = (t + 1) >> 1) {
    if (common_prefix(keys, n, i, i + (s + t) * d) > dnode) s += t;
    if (t <= 1) break;
  }
  const int gamma = i + s * d + min(d, 0);
  const int lo = min(i, j), hi = max(i, j);
  // child link: >= 0 inner node, < 0 ~leaf
  const int left = (lo == gamma) ? ~gamma : gamma;
  const int right = (hi == gamma + 1) ? ~(gamma + 1) : gamma + 1;
  children[i] = make_int2(left, right);
  parent[left >= 0 ? left : (n - 1) + ~left] = i;
  parent[right >= 0 ? right : (n - 1) + ~right] = i;
  if (i == 0) parent[0] = -1;
}

// Bottom-up passes run level by level: k_node_depth numbers every inner node with its distance from the root, then one
// launch per level (deepest first) lets each node of that level combine its two children, which the previous launch
// finished.  The kernel boundary is the only synchronisation: no arrival counters and no agent-scope fences (the
// per-XCD L2s are not coherent, cdna_hip_programming.md Guideline 16, and a fence per visited node costs an L2
// write-back: the arrival-counter version of these passes took 38 + 33 ms on 7 M triangles, this one 3 ms).
__global__ void __launch_bounds__(256) k_node_depth(int n, const int* __restrict__ parent, int* __restrict__ node_depth,
                                                    int* __restrict__ max_inner_depth, int* __restrict__ max_leaf_depth) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;   // inner nodes 0..n-2, leaf i at (n-1)+i
  if (t >= 2 * n - 1) return;
  int depth = 0;
  for (int p = parent[t]; p >= 0; p = parent[p]) ++depth;
  // one atomic per wave
  int m = depth;
  if (t >= n - 1) m = -1;
  int ml = t >= n - 1 ? depth : -1;
  for (int off = 32; off > 0; off >>= 1) {
    m = max(m, __shfl_xor(m, off));
    ml = max(ml, __shfl_xor(ml, off));
  }
  if (t < n - 1) node_depth[t] = depth;
  if ((threadIdx.x & 63) == 0) {
    if (m >= 0) atomicMax(max_inner_depth, m);
    if (ml >= 0) atomicMax(max_leaf_depth, ml);
  }
}

// One level of the bottom-up pass: boxes (FIT) and the number of inner nodes per subtree (for the depth-first layout).
template <bool FIT>
__global__ void __launch_bounds__(256) k_level_up(int n, int level, const int* __restrict__ node_depth, const int2* __restrict__ children,
                                                  float4* node_lo, float4* node_hi, int* counts) {
  const int node = blockIdx.x * blockDim.x + threadIdx.x;
  if (node >= n - 1 || node_depth[node] != level) return;
  const int2 c = children[node];
  if (FIT) {
    const int s0 = c.x >= 0 ? c.x : (n - 1) + ~c.x, s1 = c.y >= 0 ? c.y : (n - 1) + ~c.y;
    const float4 l0 = node_lo[s0], l1 = node_lo[s1];
    const float4 h0 = node_hi[s0], h1 = node_hi[s1];
    node_lo[node] = union_lo(l0, l1);
    node_hi[node] = union_hi(h0, h1);
  }
  counts[node] = 1 + (c.x >= 0 ? counts[c.x] : 0) + (c.y >= 0 ? counts[c.y] : 0);
}

// ---------------------------------------------------------------------------------------------
// PLOC (parallel locally-ordered clustering, Meister & Bittner 2018): bottom-up agglomerative build over the
// Morton-ordered leaves.  Every round each cluster looks kPlocRadius positions to both sides for the neighbour
// whose merged box has the smallest surface area; mutually nearest pairs merge into a new inner node and the
// cluster array is compacted IN ORDER (prefix sum), so it stays spatially sorted.  Optional builder
// (glz_instance_set_bvh_builder): on the atrium its trees cost the same as the Karras LBVH's overall.
// Inner-node ids are handed out downwards from n-2, so the last merge creates the root as node 0.
// ---------------------------------------------------------------------------------------------
constexpr int kPlocRadius = 16;
constexpr int kScanTile = 1024;   // elements per block of the scan kernels (256 threads x 4)

__device__ __forceinline__ int box_slot(int ref, int n) { return ref >= 0 ? ref : (n - 1) + ~ref; }

__global__ void __launch_bounds__(256) k_ploc_nearest(int m, int n, const int* __restrict__ refs, const float4* __restrict__ node_lo,
                                                      const float4* __restrict__ node_hi, int* __restrict__ nearest) {
  __shared__ float4 s_lo[256 + 2 * kPlocRadius], s_hi[256 + 2 * kPlocRadius];
  const int base = (int)(blockIdx.x * 256) - kPlocRadius;
  for (int k = threadIdx.x; k < 256 + 2 * kPlocRadius; k += 256) {
    const int idx = base + k;
    if (idx >= 0 && idx < m) {
      const int slot = box_slot(refs[idx], n);
      s_lo[k] = node_lo[slot];
      s_hi[k] = node_hi[slot];
    }
  }
  __syncthreads();
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= m) return;
  const float4 lo = s_lo[threadIdx.x + kPlocRadius], hi = s_hi[threadIdx.x + kPlocRadius];
  float best = INFINITY;
  int best_j = -1;
  for (int d = -kPlocRadius; d <= kPlocRadius; ++d) {
    const int j = i + d;
    if (d == 0 || j < 0 || j >= m) continue;
    const float4 l = s_lo[threadIdx.x + kPlocRadius + d], h = s_hi[threadIdx.x + kPlocRadius + d];
    const float dx = fmaxf(hi.x, h.x) - fminf(lo.x, l.x), dy = fmaxf(hi.y, h.y) - fminf(lo.y, l.y), dz = fmaxf(hi.z, h.z) - fminf(lo.z, l.z);
    const float area = dx * dy + dy * dz + dz * dx;
    if (area < best) {   // d ascends, so ties keep the smaller index: the globally closest pair is then always mutual
      best = area;
      best_j = j;
    }
  }
  nearest[i] = best_j;
}

// flags: low word = the cluster survives this round (merged pairs survive as their left member), high word = it is the
// left member of a merging pair (it allocates the new node)
__global__ void __launch_bounds__(256) k_ploc_flags(int m, const int* __restrict__ nearest, unsigned long long* __restrict__ flags) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= m) return;
  const int j = nearest[i];
  const bool mutual = j >= 0 && nearest[j] == i;
  const bool leader = mutual && i < j, absorbed = mutual && i > j;
  flags[i] = (absorbed ? 0ull : 1ull) | (leader ? (1ull << 32) : 0ull);
}

// exclusive prefix sum of packed counters, three phases: per-tile scan + tile totals, scan of the totals (recursive), add
__global__ void __launch_bounds__(256) k_scan_tiles(int m, const unsigned long long* __restrict__ in, unsigned long long* __restrict__ out,
                                                    unsigned long long* __restrict__ tile_sums) {
  __shared__ unsigned long long s_wave[4];
  const int base = blockIdx.x * kScanTile + threadIdx.x * 4;
  unsigned long long v[4], run = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    v[k] = base + k < m ? in[base + k] : 0ull;
    run += v[k];
  }
  unsigned long long incl = run;   // inclusive scan of the per-thread sums: wave shuffle, then the 4 wave totals
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const unsigned long long up = __shfl_up(incl, off);
    if (lane >= off) incl += up;
  }
  if (lane == 63) s_wave[wave] = incl;
  __syncthreads();
  unsigned long long before = 0;
  for (int w = 0; w < wave; ++w) before += s_wave[w];
  unsigned long long excl = before + incl - run;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (base + k < m) out[base + k] = excl;
    excl += v[k];
  }
  if (threadIdx.x == 255) tile_sums[blockIdx.x] = before + incl;
}
__global__ void __launch_bounds__(256) k_scan_add(int m, unsigned long long* __restrict__ out, const unsigned long long* __restrict__ tile_offsets) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < m) out[i] += tile_offsets[i / kScanTile];
}
// total = exclusive[m-1] + in[m-1]
__global__ void k_scan_total(int m, const unsigned long long* __restrict__ in, const unsigned long long* __restrict__ out,
                             unsigned long long* __restrict__ total) {
  if (blockIdx.x == 0 && threadIdx.x == 0) *total = out[m - 1] + in[m - 1];
}
// in/out: m elements; tmp: scratch for the tile sums of every level (>= m / 1023 + 8 elements)
static hipError_t scan_exclusive(hipStream_t st, int m, const unsigned long long* in, unsigned long long* out, unsigned long long* tmp) {
  const int tiles = (m + kScanTile - 1) / kScanTile;
  GLZ_TRY(launch(k_scan_tiles, dim3(tiles), dim3(256), st, m, in, out, tmp));
  if (tiles == 1) return hipSuccess;
  unsigned long long* sums_scanned = tmp + tiles;
  GLZ_TRY(scan_exclusive(st, tiles, tmp, sums_scanned, sums_scanned + tiles));
  return launch(k_scan_add, dim3((m + 255) / 256), dim3(256), st, m, out, sums_scanned);
}
__global__ void __launch_bounds__(256) k_ploc_merge(int m, int n, int next_free, const int* __restrict__ refs, const int* __restrict__ nearest,
                                                    const unsigned long long* __restrict__ flags, const unsigned long long* __restrict__ pos,
                                                    int* __restrict__ refs_out, int2* __restrict__ children, int* __restrict__ parent,
                                                    float4* node_lo, float4* node_hi) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= m) return;
  const unsigned long long f = flags[i], p = pos[i];
  if (!(f & 1ull)) return;   // absorbed by its left partner
  int ref = refs[i];
  if (f >> 32) {
    const int id = next_free - (int)(p >> 32);
    const int a = ref, b = refs[nearest[i]];
    const int sa = box_slot(a, n), sb = box_slot(b, n);
    const float4 l0 = node_lo[sa], l1 = node_lo[sb], h0 = node_hi[sa], h1 = node_hi[sb];
    children[id] = make_int2(a, b);
    node_lo[id] = make_float4(fminf(l0.x, l1.x), fminf(l0.y, l1.y), fminf(l0.z, l1.z), 0.0f);
    node_hi[id] = make_float4(fmaxf(h0.x, h1.x), fmaxf(h0.y, h1.y), fmaxf(h0.z, h1.z), 0.0f);
    parent[sa] = id;
    parent[sb] = id;
    ref = id;
  }
  refs_out[(uint32_t)p] = ref;
}
__global__ void __launch_bounds__(256) k_ploc_init(int n, int* __restrict__ refs, int* __restrict__ parent) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) refs[i] = ~i;
  if (i == 0) parent[0] = -1;
}

// ---- layout: depth-first (pre-order) numbering, so every subtree is one contiguous run of nodes and a node's left
// child is its neighbour.  counts[t] = inner nodes in the subtree of t (k_level_up).
__global__ void __launch_bounds__(256) k_dfs_ids(int n, const int2* __restrict__ children, const int* __restrict__ parent,
                                                 const int* __restrict__ counts, int* __restrict__ new_id) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n - 1) return;
  int id = 0;
  for (int cur = t, p = parent[t]; p >= 0; cur = p, p = parent[p]) {
    const int2 c = children[p];
    id += 1 + ((c.y == cur && c.x >= 0) ? counts[c.x] : 0);
  }
  new_id[t] = id;
}

// Quantisation grid from the root box: kBvhGridMax (32 767) cells per axis, stretched by 2^-16 so the top plane stays below it.  15 bits:
// the tracer turns a coordinate into the float 32768 + q with one byte permute (device/intersect.h box_key).
__global__ void k_grid_params(const float4* __restrict__ node_lo, const float4* __restrict__ node_hi, BvhGrid* __restrict__ grid) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const float lo[3] = {node_lo[0].x, node_lo[0].y, node_lo[0].z}, hi[3] = {node_hi[0].x, node_hi[0].y, node_hi[0].z};
  // the grid reaches kGridReach of the largest coordinate past the bounds on every side, so that the margin the boxes get at
  // quantisation (grid_margin, build_common.h) has cells to be counted in: across the thin side of a flat scene the grid is then all margin
  float largest = 0.0f;
  for (int k = 0; k < 3; ++k) largest = fmaxf(largest, fmaxf(fabsf(lo[k]), fabsf(hi[k])));
  const float reach = kGridReach * largest;
  for (int k = 0; k < 3; ++k) {
    float ext = (hi[k] - lo[k]) + 2.0f * reach;
    if (!(ext > 0.0f)) ext = 1.0f;
    const float cell = ext * 1.00002f / (float)kBvhGridMax;
    grid->lo[k] = (lo[k] - reach) - 0.5f * cell;
    grid->cell[k] = cell;
    grid->inv_cell[k] = 1.0f / cell;
  }
}
hipError_t launch_grid_params(hipStream_t st, const float4* root_lo, const float4* root_hi, BvhGrid* grid) {
  return launch(k_grid_params, dim3(1), dim3(64), st, root_lo, root_hi, grid);
}

// ---- 4-wide collapse.  A BVH4 node starts from the two children of a binary node and keeps opening the inner child
// with the LARGEST surface area (the one a ray is most likely to enter anyway) until it has four children or only leaves
// are left; an opened child's two children take its place, so the children stay in the left-to-right order of the binary
// hierarchy (the order that breaks distance ties in the tracer).  The binary nodes that head a BVH4 node are found top
// down, one launch per level of the binary hierarchy (a node marks its final children, which lie 1-3 levels below).
// flags[dfs id] = 1 for those heads, so an exclusive scan over the depth-first order numbers the BVH4 nodes depth-first.
// (Folding every odd level instead -- children = grandchildren -- left 3.0 children per node; this leaves 3.4+.)
template <int W>
struct Kids {
  int link[W];
  int n;
};
// W = 4: the nodes every tracer reads; W = 8: the 128-byte nodes of the tracer for small tile shares (types.h BvhNode8) -- the same
// rule carried on until eight children are open
template <int W>
__device__ __forceinline__ Kids<W> collapse_wide(int node, const int2* __restrict__ children, const float4* __restrict__ node_lo,
                                                 const float4* __restrict__ node_hi) {
  Kids<W> k;
  const int2 c = children[node];
  float area[W];
#pragma unroll
  for (int i = 0; i < W; ++i) { k.link[i] = kBvhEmptyChild; area[i] = -1.0f; }
  k.link[0] = c.x; k.link[1] = c.y;
  k.n = 2;
  area[0] = c.x >= 0 ? box_area(node_lo[c.x], node_hi[c.x]) : -1.0f;
  area[1] = c.y >= 0 ? box_area(node_lo[c.y], node_hi[c.y]) : -1.0f;
  while (k.n < W) {
    int j = -1;
    float best = -1.0f;
    for (int i = 0; i < W; ++i)
      if (i < k.n && k.link[i] >= 0 && area[i] > best) { best = area[i]; j = i; }   // ties: the leftmost
    if (j < 0) break;   // only leaves left
    const int2 g = children[k.link[j]];
    for (int i = W - 1; i > 0; --i)
      if (i > j + 1) { k.link[i] = k.link[i - 1]; area[i] = area[i - 1]; }
    k.link[j] = g.x; area[j] = g.x >= 0 ? box_area(node_lo[g.x], node_hi[g.x]) : -1.0f;
    k.link[j + 1] = g.y; area[j + 1] = g.y >= 0 ? box_area(node_lo[g.y], node_hi[g.y]) : -1.0f;
    ++k.n;
  }
  return k;
}
// head[t] = level of the BVH4 node headed by binary node t (root = 1), 0 = folded into an ancestor
template <int W>
__global__ void __launch_bounds__(256) k_mark_heads(int n, int level, const int* __restrict__ node_depth, const int2* __restrict__ children,
                                                    const float4* __restrict__ node_lo, const float4* __restrict__ node_hi,
                                                    int* head, int* __restrict__ max_level) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n - 1 || node_depth[t] != level) return;
  const int mine = t == 0 ? 1 : head[t];
  if (t == 0) head[0] = 1;
  if (mine == 0) return;
  const Kids<W> k = collapse_wide<W>(t, children, node_lo, node_hi);
  for (int i = 0; i < W; ++i)
    if (i < k.n && k.link[i] >= 0) head[k.link[i]] = mine + 1;
  atomicMax(max_level, mine);
}
__global__ void __launch_bounds__(256) k_head_flags(int n, const int* __restrict__ head, const int* __restrict__ new_id,
                                                    unsigned long long* __restrict__ flags) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n - 1) return;
  flags[new_id[t]] = head[t] ? 1ull : 0ull;
}

// A slot of a wide node without a child: lo = the grid's top, hi = 0 -- an inverted box no ray enters (the tracer skips the slot by its link)
__device__ __forceinline__ void empty_child_slot(uint32_t* w, uint32_t& link) {
  w[0] = w[1] = w[2] = kBvhGridMax;
  link = (uint32_t)kBvhEmptyChild;
}

__global__ void __launch_bounds__(256) k_emit_nodes4(int n, const int2* __restrict__ children, const float4* __restrict__ node_lo,
                                                     const float4* __restrict__ node_hi, const BvhGrid* __restrict__ grid,
                                                     const int* __restrict__ new_id, const unsigned long long* __restrict__ flags,
                                                     const unsigned long long* __restrict__ pos, const unsigned long long* __restrict__ slot,
                                                     uint32_t leaf_links_by_number, BvhNode4* __restrict__ nodes, float* __restrict__ sah) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n - 1) return;
  const int2 c = children[i];
  // SAH cost numerator of the binary hierarchy: surface areas of inner nodes (1.2) and leaves (1.0), normalised on the host
  float acc = 1.2f * box_area(node_lo[i], node_hi[i]);
  if (c.x < 0) acc += box_area(node_lo[(n - 1) + ~c.x], node_hi[(n - 1) + ~c.x]);
  if (c.y < 0) acc += box_area(node_lo[(n - 1) + ~c.y], node_hi[(n - 1) + ~c.y]);
  atomicAdd(sah, acc);   // reported only (the sum's order is not fixed)
  if (!flags[new_id[i]]) return;   // folded into an ancestor
  const Kids<4> kk = collapse_wide<4>(i, children, node_lo, node_hi);
  const BvhGrid g = *grid;
  float gm[3];
  grid_margin(g, gm);
  BvhNode4 nd;
  for (int k = 0; k < 4; ++k) {
    const int ch = kk.link[k];
    if (k >= kk.n) {
      empty_child_slot(&nd.w[3 * k], nd.w[12 + k]);
      continue;
    }
    const int box = ch >= 0 ? ch : (n - 1) + ~ch;
    const float4 l = node_lo[box], h = node_hi[box];
    const uint32_t q[6] = {quant_lo(l.x, g.lo[0], g.inv_cell[0], gm[0]), quant_lo(l.y, g.lo[1], g.inv_cell[1], gm[1]), quant_lo(l.z, g.lo[2], g.inv_cell[2], gm[2]),
                           quant_hi(h.x, g.lo[0], g.inv_cell[0], gm[0]), quant_hi(h.y, g.lo[1], g.inv_cell[1], gm[1]), quant_hi(h.z, g.lo[2], g.inv_cell[2], gm[2])};
    nd.w[3 * k] = q[0] | (q[3] << 16);       // one word per axis: lo | hi << 16 (build_common.h quant_box)
    nd.w[3 * k + 1] = q[1] | (q[4] << 16);
    nd.w[3 * k + 2] = q[2] | (q[5] << 16);
    // inner: its number among the BVH4 nodes; leaf: ~(first slot of the leaf in bvh_tris), or ~(leaf number) when the tracer reads
    // per-leaf records that name the slot (HierarchyInputs::emit_quads)
    nd.w[12 + k] = (uint32_t)(ch >= 0 ? (int)pos[new_id[ch]] : (leaf_links_by_number ? ch : ~(int)slot[~ch]));
  }
  nodes[pos[new_id[i]]] = nd;
}

// The same hierarchy collapsed eight wide (types.h BvhNode8): heads found by k_mark_heads<8>, numbered depth-first like the 4-wide
// nodes; same grid, same padding, leaf links by leaf number (only the flattened build with per-leaf records carries these nodes).
__global__ void __launch_bounds__(256) k_emit_nodes8(int n, const int2* __restrict__ children, const float4* __restrict__ node_lo,
                                                     const float4* __restrict__ node_hi, const BvhGrid* __restrict__ grid,
                                                     const int* __restrict__ new_id, const unsigned long long* __restrict__ flags,
                                                     const unsigned long long* __restrict__ pos, BvhNode8* __restrict__ nodes) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n - 1 || !flags[new_id[i]]) return;
  const Kids<8> kk = collapse_wide<8>(i, children, node_lo, node_hi);
  const BvhGrid g = *grid;
  float gm[3];
  grid_margin(g, gm);
  BvhNode8 nd;
  for (int k = 0; k < 8; ++k) {
    const int ch = kk.link[k];
    if (k >= kk.n) {
      empty_child_slot(&nd.w[3 * k], nd.w[24 + k]);
      continue;
    }
    const int box = ch >= 0 ? ch : (n - 1) + ~ch;
    const float4 l = node_lo[box], h = node_hi[box];
    quant_box(l, h, g, gm, &nd.w[3 * k]);
    nd.w[24 + k] = (uint32_t)(ch >= 0 ? (int)pos[new_id[ch]] : ch);
  }
  nodes[pos[new_id[i]]] = nd;
}

// Leaves from given boxes (HierarchyInputs::given_lo / given_hi): the box arrays the rest of the build works on, a placeholder
// triangle per box that carries its index, and the bounds of the box centres.
__global__ void __launch_bounds__(256) k_given_boxes(const float4* __restrict__ glo, const float4* __restrict__ ghi, uint32_t n, BvhTri* __restrict__ tris,
                                                     float4* __restrict__ box_lo, float4* __restrict__ box_hi, int* __restrict__ scene_bounds) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float4 l = glo[i], h = ghi[i];
  BvhTri t{};
  t.world_id = i;
  t.instance = i;
  tris[i] = t;
  box_lo[i] = make_float4(l.x, l.y, l.z, 0.0f);
  box_hi[i] = make_float4(h.x, h.y, h.z, 0.0f);
  float c[3];
  box_centroid(l, h, c);
#pragma unroll
  for (int k = 0; k < 3; ++k) {   // one atomic pair per box: instance counts are small next to triangle counts
    atomicMin(&scene_bounds[k], float_to_ordered(c[k]));
    atomicMax(&scene_bounds[3 + k], float_to_ordered(c[k]));
  }
}

// ---------------------------------------------------------------------------------------------
// host side: the stages of a build, one function each, and build_hierarchy, which runs them
// ---------------------------------------------------------------------------------------------
static uint32_t next_pow2(uint32_t v) {
  uint32_t p = 1;
  while (p < v) p <<= 1;
  return p;
}

// What the stages share: the binary hierarchy over the leaf boxes, the arrays of the scans and the build's scalars.  Like every
// temporary of the build it is freed on the way out, whichever way that is (hipFree waits for work in flight).
struct BuildWorkspace {
  DeviceBuffer<float4> node_lo, node_hi;   // boxes: inner node i at slot i, leaf j (in sorted order) at slot (n-1)+j
  DeviceBuffer<int2> children;             // of inner node i; a link >= 0 is an inner node, < 0 ~leaf
  DeviceBuffer<int> parent;                // by box slot; -1 for the root
  DeviceBuffer<uint64_t> keys;             // the leaves' Morton codes, sorted (the LBVH's input)
  DeviceBuffer<unsigned long long> flags, pos, slot, scan_tmp, scan_total;   // a scan's input and result; first slot of every leaf in bvh_tris; scratch
  DeviceBuffer<int> scalars;               // [0..5] ordered-int bounds of the leaf centres, [6] depth of the deepest leaf, [7] depth counter of the pass at hand
  DeviceBuffer<float> sah;                 // SAH cost numerator (k_emit_nodes4)
  DeviceBuffer<BvhGrid> grid;

  hipError_t alloc(uint32_t nw) {
    const size_t tiles = ((size_t)nw + kScanTile - 1) / kScanTile, np_max = std::max<uint32_t>(next_pow2(nw), kSortTile);
    GLZ_TRY(alloc_each(2 * (size_t)nw, node_lo, node_hi, parent));
    GLZ_TRY(alloc_each(nw, children, flags, pos, slot));
    GLZ_TRY(keys.alloc(np_max));
    GLZ_TRY(scan_tmp.alloc(2 * tiles + 4096));
    GLZ_TRY(alloc_each(1, scan_total, sah, grid));
    return scalars.alloc(8);
  }
};

// Exclusive scan of ws.flags[0..m) into ws.pos, and the sum of all m elements on its way to *host_total: it is there after the caller's
// next synchronisation of the stream
static hipError_t scan_with_total(hipStream_t st, int m, BuildWorkspace& ws, unsigned long long* host_total) {
  GLZ_TRY(scan_exclusive(st, m, ws.flags.ptr, ws.pos.ptr, ws.scan_tmp.ptr));
  GLZ_TRY(launch(k_scan_total, dim3(1), dim3(64), st, m, ws.flags.ptr, ws.pos.ptr, ws.scan_total.ptr));
  return hipMemcpyAsync(host_total, ws.scan_total.ptr, sizeof(*host_total), hipMemcpyDeviceToHost, st);
}

// The arrays of the leaves stage alone.  build_hierarchy owns them so that they last as long as the build: freeing them at the end of
// their stage would make the host wait for the device in the middle of a build, with the builder's launches not yet queued.
struct LeafArrays {
  DeviceBuffer<BvhTri> tris_unsorted;      // by world triangle (or given box)
  DeviceBuffer<float4> lo, hi;             // their boxes
  DeviceBuffer<uint8_t> role;              // k_pair_triangles
  DeviceBuffer<uint32_t> leaf_first;       // leaf (numbered in world-triangle order) -> its first triangle
  DeviceBuffer<float4> leaf_lo, leaf_hi;   // ... -> its box
  DeviceBuffer<uint32_t> vals;             // leaf numbers, sorted with the Morton codes
};

// Leaves: world triangles (or the given boxes), pairs of triangles where they qualify and single triangles otherwise, Morton codes,
// sort, and the gather into leaf order -- out.tris, out.quads, the leaf boxes in ws.node_lo / node_hi, ws.slot.  n: the number of leaves.
static hipError_t build_leaves(hipStream_t st, const HierarchyInputs& in, LeafArrays& l, BuildWorkspace& ws, HierarchyOutputs& out, uint32_t& n) {
  const uint32_t nw = in.n_world;
  GLZ_TRY(alloc_each(nw, l.tris_unsorted, l.lo, l.hi, l.role, l.leaf_first, l.leaf_lo, l.leaf_hi));
  GLZ_TRY(l.vals.alloc(ws.keys.count));
  GLZ_TRY(hipMemsetAsync(l.role.ptr, 0, nw, st));
  // ordered-int encodings of +inf / -inf, then the two depth counters
  static const int init[8] = {0x7F800000, 0x7F800000, 0x7F800000, (int)0xFF800000 ^ 0x7FFFFFFF, (int)0xFF800000 ^ 0x7FFFFFFF, (int)0xFF800000 ^ 0x7FFFFFFF, 0, 0};
  GLZ_TRY(hipMemcpyAsync(ws.scalars.ptr, init, sizeof(init), hipMemcpyHostToDevice, st));
  const dim3 blk(256), grdw((nw + 255) / 256);
  if (in.given_lo && in.given_hi)
    GLZ_TRY(launch(k_given_boxes, grdw, blk, st, in.given_lo, in.given_hi, nw, l.tris_unsorted.ptr, l.lo.ptr, l.hi.ptr, ws.scalars.ptr));
  else
    GLZ_TRY(launch(k_world_tris, grdw, blk, st, in.vertices, in.indices, in.instances, in.inst_base, in.n_instances, in.transforms, in.materials, nw,
                   l.tris_unsorted.ptr, l.lo.ptr, l.hi.ptr, ws.scalars.ptr));
  // leaves: pairs of triangles where they qualify, single triangles otherwise
  if (in.pair_area_ratio > 0.0f && !in.given_lo)
    for (uint32_t parity = 0; parity < 2; ++parity)
      GLZ_TRY(launch(k_pair_triangles, grdw, blk, st, nw, parity, l.tris_unsorted.ptr, in.indices, in.instances, l.lo.ptr, l.hi.ptr, in.pair_area_ratio,
                     in.emit_quads ? 1u : 0u, l.role.ptr));
  GLZ_TRY(launch(k_leaf_flags, grdw, blk, st, nw, l.role.ptr, ws.flags.ptr));
  unsigned long long n_leaves = 0;
  GLZ_TRY(scan_with_total(st, (int)nw, ws, &n_leaves));
  GLZ_TRY(hipStreamSynchronize(st));
  n = (uint32_t)n_leaves;
  if (n == 0 || n > nw) return hipErrorUnknown;
  GLZ_TRY(launch(k_leaf_boxes, grdw, blk, st, nw, l.role.ptr, ws.pos.ptr, l.lo.ptr, l.hi.ptr, l.leaf_first.ptr, l.leaf_lo.ptr, l.leaf_hi.ptr));
  const uint32_t np = std::max<uint32_t>(next_pow2(n), kSortTile);
  const dim3 grd((n + 255) / 256);
  uint64_t* keys = ws.keys.ptr;
  uint32_t* vals = l.vals.ptr;   // leaf numbers: they travel with their keys
  GLZ_TRY(launch(k_morton, dim3((np + 255) / 256), blk, st, l.leaf_lo.ptr, l.leaf_hi.ptr, ws.scalars.ptr, n, np, keys, vals));
  // bitonic network: stages k = 2..np; strides j = k/2..1
  GLZ_TRY(launch(k_bitonic_lds, dim3(np / kSortTile), dim3(1024), st, keys, vals, np, 2u, kSortTile, 0u));
  for (uint32_t k = kSortTile * 2; k <= np; k <<= 1) {
    for (uint32_t j = k >> 1; j >= kSortTile; j >>= 1) GLZ_TRY(launch(k_bitonic_global, dim3((np / 2 + 255) / 256), blk, st, keys, vals, np, k, j));
    GLZ_TRY(launch(k_bitonic_lds, dim3(np / kSortTile), dim3(1024), st, keys, vals, np, k, k, kSortTile / 2));
  }
  // first slot of every leaf in bvh_tris (leaf order, one or two triangles each)
  GLZ_TRY(launch(k_leaf_sizes, grd, blk, st, n, vals, l.leaf_first.ptr, l.role.ptr, ws.flags.ptr));
  GLZ_TRY(scan_exclusive(st, (int)n, ws.flags.ptr, ws.slot.ptr, ws.scan_tmp.ptr));
  if (in.emit_quads) GLZ_TRY(out.quads.alloc(n));
  return launch(k_gather_leaves, grd, blk, st, vals, n, l.leaf_first.ptr, l.role.ptr, ws.slot.ptr, l.tris_unsorted.ptr, l.leaf_lo.ptr, l.leaf_hi.ptr, out.tris,
                ws.node_lo.ptr, ws.node_hi.ptr, out.quads.ptr);
}

// ---- the binary hierarchy over n >= 2 leaves, one function per builder: each fills ws.children / ws.parent (PLOC the inner boxes too) ----
static hipError_t build_lbvh(hipStream_t st, uint32_t n, BuildWorkspace& ws) {
  return launch(k_hierarchy, dim3((n + 255) / 256), dim3(256), st, ws.keys.ptr, (int)n, ws.children.ptr, ws.parent.ptr);
}

static hipError_t build_ploc(hipStream_t st, uint32_t n, BuildWorkspace& ws) {
  DeviceBuffer<int> refs_a, refs_b, nearest;
  GLZ_TRY(alloc_each(n, refs_a, refs_b, nearest));
  const dim3 blk(256);
  GLZ_TRY(launch(k_ploc_init, dim3((n + 255) / 256), blk, st, (int)n, refs_a.ptr, ws.parent.ptr));
  int m = (int)n, next_free = (int)n - 2;
  while (m > 1) {
    const dim3 gm((m + 255) / 256);
    GLZ_TRY(launch(k_ploc_nearest, gm, blk, st, m, (int)n, refs_a.ptr, ws.node_lo.ptr, ws.node_hi.ptr, nearest.ptr));
    GLZ_TRY(launch(k_ploc_flags, gm, blk, st, m, nearest.ptr, ws.flags.ptr));
    unsigned long long total = 0;
    GLZ_TRY(scan_with_total(st, m, ws, &total));
    GLZ_TRY(launch(k_ploc_merge, gm, blk, st, m, (int)n, next_free, refs_a.ptr, nearest.ptr, ws.flags.ptr, ws.pos.ptr, refs_b.ptr, ws.children.ptr, ws.parent.ptr,
                   ws.node_lo.ptr, ws.node_hi.ptr));
    GLZ_TRY(hipStreamSynchronize(st));
    const int survivors = (int)(total & 0xFFFFFFFFull), merges = (int)(total >> 32);
    if (merges <= 0 || survivors != m - merges) return hipErrorUnknown;   // cannot happen: the closest pair is always mutual
    next_free -= merges;
    m = survivors;
    std::swap(refs_a, refs_b);
  }
  return hipSuccess;
}

// the SAH builder on the host cores (bvh_sah.cpp): the reference the GPU builder is tested against
static hipError_t build_sah_on_host(hipStream_t st, uint32_t n, BuildWorkspace& ws) {
  std::vector<float4> h_lo(n), h_hi(n);
  std::vector<int2> h_children(n);
  std::vector<int> h_parent(2 * (size_t)n);
  GLZ_TRY(hipMemcpyAsync(h_lo.data(), ws.node_lo.ptr + (n - 1), sizeof(float4) * n, hipMemcpyDeviceToHost, st));
  GLZ_TRY(hipMemcpyAsync(h_hi.data(), ws.node_hi.ptr + (n - 1), sizeof(float4) * n, hipMemcpyDeviceToHost, st));
  GLZ_TRY(hipStreamSynchronize(st));
  build_sah_host(n, h_lo.data(), h_hi.data(), h_children.data(), h_parent.data());
  GLZ_TRY(hipMemcpyAsync(ws.children.ptr, h_children.data(), sizeof(int2) * (n - 1), hipMemcpyHostToDevice, st));
  GLZ_TRY(hipMemcpyAsync(ws.parent.ptr, h_parent.data(), sizeof(int) * (2 * (size_t)n - 1), hipMemcpyHostToDevice, st));
  return hipStreamSynchronize(st);
}

// ---- finish: what follows any builder ----
// The collapse, 4 wide and 8 wide alike: finds the heads of the W-wide nodes top down and numbers them in depth-first order (ws.flags ->
// ws.pos, which the emit kernel of that width reads); gives how many W-wide nodes there are and how deep they nest.
template <int W>
static hipError_t count_heads(hipStream_t st, uint32_t n, int inner_depth, const int* node_depth, const int* new_id, int* head, BuildWorkspace& ws,
                              uint32_t& n_heads, uint32_t& depth) {
  const dim3 blk(256), grd((n + 255) / 256);
  int* deepest_head = ws.scalars.ptr + 7;
  GLZ_TRY(hipMemsetAsync(head, 0, sizeof(int) * n, st));
  GLZ_TRY(hipMemsetAsync(deepest_head, 0, sizeof(int), st));
  for (int level = 0; level <= inner_depth; ++level)
    GLZ_TRY(launch(k_mark_heads<W>, grd, blk, st, (int)n, level, node_depth, ws.children.ptr, ws.node_lo.ptr, ws.node_hi.ptr, head, deepest_head));
  GLZ_TRY(launch(k_head_flags, grd, blk, st, (int)n, head, new_id, ws.flags.ptr));
  unsigned long long total = 0;
  int deepest = 0;
  GLZ_TRY(scan_with_total(st, (int)n - 1, ws, &total));
  GLZ_TRY(hipMemcpyAsync(&deepest, deepest_head, sizeof(int), hipMemcpyDeviceToHost, st));
  GLZ_TRY(hipStreamSynchronize(st));
  n_heads = (uint32_t)total;
  depth = (uint32_t)deepest;
  return hipSuccess;
}

// Node depths, the bottom-up pass (boxes where the builder left that to it, subtree sizes), depth-first ids, the grid, and the wide
// nodes: out.nodes / out.depth and, on request, out.nodes8 / out.depth8.  Its three arrays are freed on return, right behind the last emit
// launch: hipFree waits for that launch, a wait the read-back's synchronisation that follows would otherwise have had.
static hipError_t finish_hierarchy(hipStream_t st, const HierarchyInputs& in, uint32_t n, bool fit_boxes, BuildWorkspace& ws, HierarchyOutputs& out) {
  DeviceBuffer<int> node_depth, counts, new_id;
  GLZ_TRY(alloc_each(n, node_depth, counts, new_id));
  const dim3 blk(256), grd((n + 255) / 256);
  int2* children = ws.children.ptr;
  float4 *node_lo = ws.node_lo.ptr, *node_hi = ws.node_hi.ptr;
  // bottom-up, one launch per level: boxes (LBVH; PLOC made them while merging) and subtree sizes
  GLZ_TRY(launch(k_node_depth, dim3((2 * n + 255) / 256), blk, st, (int)n, ws.parent.ptr, node_depth.ptr, ws.scalars.ptr + 7, ws.scalars.ptr + 6));
  int inner_depth = 0;
  GLZ_TRY(hipMemcpyAsync(&inner_depth, ws.scalars.ptr + 7, sizeof(int), hipMemcpyDeviceToHost, st));
  GLZ_TRY(hipStreamSynchronize(st));
  for (int level = inner_depth; level >= 0; --level)
    GLZ_TRY(launch(fit_boxes ? k_level_up<true> : k_level_up<false>, grd, blk, st, (int)n, level, node_depth.ptr, children, node_lo, node_hi, counts.ptr));
  // depth-first layout of the finished hierarchy
  GLZ_TRY(launch(k_dfs_ids, grd, blk, st, (int)n, children, ws.parent.ptr, counts.ptr, new_id.ptr));
  GLZ_TRY(launch(k_grid_params, dim3(1), dim3(64), st, node_lo, node_hi, ws.grid.ptr));
  int* head = counts.ptr;   // k_dfs_ids was the last reader of the subtree sizes
  // 4-wide collapse: heads, depth-first numbers, then emit the nodes
  uint32_t n4 = 0;
  GLZ_TRY(count_heads<4>(st, n, inner_depth, node_depth.ptr, new_id.ptr, head, ws, n4, out.depth));
  GLZ_TRY(out.nodes.alloc(n4));
  GLZ_TRY(launch(k_emit_nodes4, grd, blk, st, (int)n, children, node_lo, node_hi, ws.grid.ptr, new_id.ptr, ws.flags.ptr, ws.pos.ptr, ws.slot.ptr,
                 in.emit_quads ? 1u : 0u, out.nodes.ptr, ws.sah.ptr));
  if (in.emit_wide8 && in.emit_quads) {
    // the 8-wide collapse of the same binary hierarchy: heads, depth-first numbers, nodes (head / flags / pos are free again)
    uint32_t n8 = 0;
    GLZ_TRY(count_heads<8>(st, n, inner_depth, node_depth.ptr, new_id.ptr, head, ws, n8, out.depth8));
    GLZ_TRY(out.nodes8.alloc(n8));
    GLZ_TRY(launch(k_emit_nodes8, grd, blk, st, (int)n, children, node_lo, node_hi, ws.grid.ptr, new_id.ptr, ws.flags.ptr, ws.pos.ptr, out.nodes8.ptr));
  }
  return hipSuccess;
}

// The scene of one leaf: one node whose first child is leaf 0 with a box spanning the whole grid
static hipError_t one_leaf_scene(hipStream_t st, BuildWorkspace& ws, HierarchyOutputs& out) {
  GLZ_TRY(launch(k_grid_params, dim3(1), dim3(64), st, ws.node_lo.ptr, ws.node_hi.ptr, ws.grid.ptr));   // slot (n-1)+0 = 0 is the leaf box
  BvhNode4 nd = childless_node4();
  nd.w[0] = nd.w[1] = nd.w[2] = 0u | (kBvhGridMax << 16);   // lo 0, hi the grid's top on every axis
  nd.w[12] = ~0u;   // leaf 0
  GLZ_TRY(out.nodes.alloc(1));
  GLZ_TRY(hipMemcpyAsync(out.nodes.ptr, &nd, sizeof(nd), hipMemcpyHostToDevice, st));
  GLZ_TRY(hipStreamSynchronize(st));
  out.depth = 1;   // levels of 4-wide nodes above the deepest leaf
  return hipSuccess;
}

// bounds (box slot 0: the root, or the only leaf) and the SAH cost: the sum of k_emit_nodes4 over the root's area (0 for one leaf)
static hipError_t read_back_bounds_and_cost(hipStream_t st, BuildWorkspace& ws, HierarchyOutputs& out) {
  float host_sah = 0.0f;
  float4 root_lo, root_hi;
  GLZ_TRY(hipMemcpyAsync(&host_sah, ws.sah.ptr, sizeof(float), hipMemcpyDeviceToHost, st));
  GLZ_TRY(hipMemcpyAsync(&root_lo, ws.node_lo.ptr, sizeof(float4), hipMemcpyDeviceToHost, st));
  GLZ_TRY(hipMemcpyAsync(&root_hi, ws.node_hi.ptr, sizeof(float4), hipMemcpyDeviceToHost, st));
  GLZ_TRY(hipStreamSynchronize(st));
  const float ra = box_area(root_lo, root_hi);
  out.sah = ra > 0.0f ? host_sah / ra : 0.0f;
  out.bounds_lo[0] = root_lo.x; out.bounds_lo[1] = root_lo.y; out.bounds_lo[2] = root_lo.z;
  out.bounds_hi[0] = root_hi.x; out.bounds_hi[1] = root_hi.y; out.bounds_hi[2] = root_hi.z;
  return hipSuccess;
}

hipError_t build_hierarchy(hipStream_t st, const HierarchyInputs& in, HierarchyOutputs& out) {
  const int builder = in.builder == kBvhBuilderAuto ? kBvhBuilderSah : in.builder;
  out.depth = out.depth8 = 0;
  out.sah = 0.0f;
  out.nodes.release();
  out.nodes8.release();
  out.quads.release();
  if (in.n_world == 0) return hipSuccess;
  BuildWorkspace ws;
  LeafArrays leaves;
  GLZ_TRY(ws.alloc(in.n_world));
  GLZ_TRY(hipMemsetAsync(ws.sah.ptr, 0, sizeof(float), st));
  uint32_t n = 0;   // leaves of the hierarchy <= world triangles
  GLZ_TRY(build_leaves(st, in, leaves, ws, out, n));
  if (n >= 2) {
    if (builder == kBvhBuilderLbvh) GLZ_TRY(build_lbvh(st, n, ws));
    else if (builder == kBvhBuilderSah) GLZ_TRY(build_sah_levels(st, n, ws.node_lo.ptr + (n - 1), ws.node_hi.ptr + (n - 1), ws.children.ptr, ws.parent.ptr));
    else if (builder == kBvhBuilderSahHost) GLZ_TRY(build_sah_on_host(st, n, ws));
    else GLZ_TRY(build_ploc(st, n, ws));
    GLZ_TRY(finish_hierarchy(st, in, n, builder != kBvhBuilderPloc, ws, out));
  }
  GLZ_TRY(read_back_bounds_and_cost(st, ws, out));
  if (n == 1) GLZ_TRY(one_leaf_scene(st, ws, out));
  return hipMemcpy(&out.grid, ws.grid.ptr, sizeof(BvhGrid), hipMemcpyDeviceToHost);   // (after the one leaf's k_grid_params)
}

}  // namespace glz
