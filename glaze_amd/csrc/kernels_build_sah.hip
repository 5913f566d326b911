// The binned SAH builder of the scene build for gfx950: one block per node where ranges are short, several blocks per node where they
// are long, and the level loop that drives both (build_sah_levels, called by build_hierarchy in kernels_build.hip).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "build_common.h"
#include "device_buffer.h"

namespace glz {

// ---------------------------------------------------------------------------------------------
// Top-down binned SAH on the GPU (GLZ_BVH_SAH): the same algorithm, arithmetic and tie-breaks as the host reference in
// bvh_sah.cpp, so both give the same tree node for node (tests/test_gpu_scene_trace.py).  One launch per level, one block
// per node of the level: centroid bounds of the node's range (LDS reduction) -> 3 x 16 bins (LDS atomics on ordered-int
// box coordinates) -> thread 0 walks the 45 candidate splits exactly as the host does -> stable partition of the range
// into the other index array (block-wide prefix sums over tiles) -> children.  A subtree over c leaves owns c - 1
// consecutive node ids (left child id + 1, right child id + c_left), so ids do not depend on which block runs when.
// The top levels are few blocks over long ranges (level 0 of 131 k leaves: 1.5 ms), the rest is wide and short.
// ---------------------------------------------------------------------------------------------
constexpr int kSahBins = 16;
struct SahTask {
  uint32_t b, e;
  int node;
};
__device__ __forceinline__ int sah_bin_of(float c, float lo, float scale) {
  const float f = (c - lo) * scale;
  return f >= 0.0f ? (f < (float)kSahBins ? (int)f : kSahBins - 1) : 0;
}
// surface area of the box over a run of bins; an empty run (lo = +inf, hi = -inf) has none: part of the split rule
__device__ __forceinline__ float sah_area(const float* lo, const float* hi) {
  return hi[0] - lo[0] < 0.0f ? 0.0f : box_area(make_float4(lo[0], lo[1], lo[2], 0.0f), make_float4(hi[0], hi[1], hi[2], 0.0f));
}
// ---- passes over a range of the index array that the one-block and the several-blocks kernels share ----
// empties the 3 x kSahBins bins: entries first, first + stride, ...
__device__ __forceinline__ void sah_reset_bins(int* box, uint32_t* count, int first, int stride) {
  for (int i = first; i < 3 * kSahBins * 6; i += stride) box[i] = (i % 6) < 3 ? float_to_ordered(INFINITY) : float_to_ordered(-INFINITY);
  for (int i = first; i < 3 * kSahBins; i += stride) count[i] = 0;
}
// one leaf into its bin on every axis that has an extent
__device__ __forceinline__ void sah_bin_leaf(float4 l, float4 h, const float* clo, const float* scale, int* box, uint32_t* count) {
  float c[3];
  box_centroid(l, h, c);
  for (int a = 0; a < 3; ++a) {
    if (!(scale[a] > 0.0f)) continue;
    const int k = a * kSahBins + sah_bin_of(c[a], clo[a], scale[a]);
    int* bx = box + k * 6;
    atomicMin(&bx[0], float_to_ordered(l.x)); atomicMin(&bx[1], float_to_ordered(l.y)); atomicMin(&bx[2], float_to_ordered(l.z));
    atomicMax(&bx[3], float_to_ordered(h.x)); atomicMax(&bx[4], float_to_ordered(h.y)); atomicMax(&bx[5], float_to_ordered(h.z));
    atomicAdd(&count[k], 1u);
  }
}
// Centroid bounds of the elements [begin, end) over a block of B threads (one barrier): threads 0, 1, 2 get the bounds on x, y, z in
// l, h.  s_red: [lo xyz, hi xyz][wave]
template <int B>
__device__ __forceinline__ void sah_block_centroid_bounds(uint32_t begin, uint32_t end, const uint32_t* __restrict__ idx_in, const float4* __restrict__ leaf_lo,
                                                          const float4* __restrict__ leaf_hi, float (*s_red)[B / 64], float& l, float& h) {
  const int tid = threadIdx.x;
  float clo[3] = {INFINITY, INFINITY, INFINITY}, chi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (uint32_t i = begin + tid; i < end; i += B) {
    const uint32_t p = idx_in[i];
    float c[3];
    box_centroid(leaf_lo[p], leaf_hi[p], c);
    for (int k = 0; k < 3; ++k) { clo[k] = fminf(clo[k], c[k]); chi[k] = fmaxf(chi[k], c[k]); }
  }
  for (int off = 32; off > 0; off >>= 1)
    for (int k = 0; k < 3; ++k) { clo[k] = fminf(clo[k], __shfl_xor(clo[k], off)); chi[k] = fmaxf(chi[k], __shfl_xor(chi[k], off)); }
  if ((tid & 63) == 0)
    for (int k = 0; k < 3; ++k) { s_red[k][tid >> 6] = clo[k]; s_red[3 + k][tid >> 6] = chi[k]; }
  __syncthreads();
  l = INFINITY; h = -INFINITY;
  if (tid < 3)
    for (int w = 0; w < B / 64; ++w) { l = fminf(l, s_red[tid][w]); h = fmaxf(h, s_red[3 + tid][w]); }
}
// sum of `mine` over a block of B threads (one barrier); the total is thread 0's, the other threads get 0.  s_sum: B / 64 words
template <int B>
__device__ __forceinline__ uint32_t sah_block_sum(uint32_t mine, uint32_t* s_sum) {
  const int tid = threadIdx.x;
  for (int off = 32; off > 0; off >>= 1) mine += __shfl_xor(mine, off);
  if ((tid & 63) == 0) s_sum[tid >> 6] = mine;
  __syncthreads();
  uint32_t total = 0;
  if (tid == 0)
    for (int k = 0; k < B / 64; ++k) total += s_sum[k];
  return total;
}
// The split of a node from its bins: bvh_sah.cpp, Builder::split, statement for statement (candidate order, strict '<').
// box: [3][kSahBins][6] ordered-int lo xyz / hi xyz, count: [3][kSahBins]; axis < 0 when binning separates nothing.
// (Inlined by force: as a call that returns its result in memory it took 292 bytes of scratch in k_sah_level.)
struct SahSplit { int axis, bin; uint32_t n_left; };   // n_left: elements in the bins 0..bin of the axis
__device__ __forceinline__ SahSplit sah_pick_split(const int* box, const uint32_t* count, const float* scale) {
  float best_cost = INFINITY;
  int best_axis = -1, best_bin = -1;
  for (int a = 0; a < 3; ++a) {
    if (!(scale[a] > 0.0f)) continue;
    const int* bx = box + a * kSahBins * 6;
    const uint32_t* cn = count + a * kSahBins;
    float right_area[kSahBins];
    uint32_t right_cnt[kSahBins];
    float alo[3] = {INFINITY, INFINITY, INFINITY}, ahi[3] = {-INFINITY, -INFINITY, -INFINITY};
    uint32_t c = 0;
    for (int k = kSahBins - 1; k > 0; --k) {
      for (int d = 0; d < 3; ++d) { alo[d] = fminf(alo[d], ordered_to_float(bx[k * 6 + d])); ahi[d] = fmaxf(ahi[d], ordered_to_float(bx[k * 6 + 3 + d])); }
      c += cn[k];
      right_area[k] = sah_area(alo, ahi);
      right_cnt[k] = c;
    }
    for (int d = 0; d < 3; ++d) { alo[d] = INFINITY; ahi[d] = -INFINITY; }
    c = 0;
    for (int k = 0; k < kSahBins - 1; ++k) {
      for (int d = 0; d < 3; ++d) { alo[d] = fminf(alo[d], ordered_to_float(bx[k * 6 + d])); ahi[d] = fmaxf(ahi[d], ordered_to_float(bx[k * 6 + 3 + d])); }
      c += cn[k];
      if (c == 0 || right_cnt[k + 1] == 0) continue;
      const float cost = sah_area(alo, ahi) * (float)c + right_area[k + 1] * (float)right_cnt[k + 1];
      if (cost < best_cost) { best_cost = cost; best_axis = a; best_bin = k; }
    }
  }
  uint32_t n_left = 0;
  if (best_axis >= 0)
    for (int k = 0; k <= best_bin; ++k) n_left += count[best_axis * kSahBins + k];
  return SahSplit{best_axis, best_bin, n_left};
}
// The two children of node t once its range is in order in idx_out: a leaf is linked, a longer range gets the next node id of the
// subtree and goes to `defer` (the next level's queue, or the stack of a block that finishes the subtree by itself).
template <class Defer>
__device__ __forceinline__ void sah_link_children(const SahTask& t, uint32_t mid, const uint32_t* idx_out, int n_leaves, int2* children, int* parent, Defer defer) {
  int link[2];
  const uint32_t rb[2] = {t.b, mid}, re[2] = {mid, t.e};
  int next_id = t.node + 1;
  for (int s = 0; s < 2; ++s) {
    const uint32_t c = re[s] - rb[s];
    if (c == 1) {
      const uint32_t leaf = idx_out[rb[s]];
      link[s] = ~(int)leaf;
      parent[(n_leaves - 1) + (int)leaf] = t.node;
    } else {
      link[s] = next_id;
      parent[next_id] = t.node;
      defer(SahTask{rb[s], re[s], next_id});
      next_id += (int)c - 1;
    }
  }
  children[t.node] = make_int2(link[0], link[1]);
}
// ... with the longer ranges queued for the next level
__device__ inline void sah_emit_children(const SahTask& t, uint32_t mid, const uint32_t* idx_out, int n_leaves, int2* children, int* parent,
                                         SahTask* queue_out, uint32_t* n_out) {
  sah_link_children(t, mid, idx_out, n_leaves, children, parent, [=](const SahTask& child) { queue_out[atomicAdd(n_out, 1u)] = child; });
}
// Stable partition of the elements [begin, end) of node t (a whole range or one chunk of it) into idx_out: lefts go to
// t.b + done_left..., rights to mid + done_right..., a tile of B elements at a time.  s_wave_sum: B / 64 words, s_done: 2.
template <int B>
__device__ inline void sah_scatter(uint32_t begin, uint32_t end, uint32_t node_b, uint32_t mid, int axis, int bin, float lo_a, float scale_a,
                                   uint32_t done_left, uint32_t done_right, const uint32_t* __restrict__ idx_in, uint32_t* __restrict__ idx_out,
                                   const float4* __restrict__ leaf_lo, const float4* __restrict__ leaf_hi, uint32_t* s_wave_sum, uint32_t* s_done) {
  const int tid = threadIdx.x;
  if (tid == 0) { s_done[0] = done_left; s_done[1] = done_right; }
  __syncthreads();
  for (uint32_t base = begin; base < end; base += B) {
    const uint32_t i = base + tid;
    uint32_t p = 0;
    bool left = false;
    const bool valid = i < end;
    if (valid) {
      p = idx_in[i];
      left = sah_bin_of(box_centroid(leaf_lo[p], leaf_hi[p], axis), lo_a, scale_a) <= bin;
    }
    const unsigned long long m = __ballot(valid && left);
    const uint32_t in_wave = (uint32_t)__popcll(m & ((1ull << (tid & 63)) - 1ull));
    if ((tid & 63) == 0) s_wave_sum[tid >> 6] = (uint32_t)__popcll(m);
    __syncthreads();
    uint32_t before = 0, tile_left = 0;
    for (int w = 0; w < B / 64; ++w) {
      if (w < (tid >> 6)) before += s_wave_sum[w];
      tile_left += s_wave_sum[w];
    }
    const uint32_t lpos = before + in_wave;                 // lefts of the tile before this element
    if (valid) {
      if (left) idx_out[node_b + s_done[0] + lpos] = p;
      else idx_out[mid + s_done[1] + ((uint32_t)tid - lpos)] = p;
    }
    __syncthreads();
    if (tid == 0) {
      const uint32_t tile = min((uint32_t)B, end - base);
      s_done[0] += tile_left;
      s_done[1] += tile - tile_left;
    }
    __syncthreads();
  }
}

// One block per node of the level.  A one-wave block whose node holds at most 64 leaves finishes the whole subtree by
// itself (children go on a stack in LDS, each reading the index array its parent wrote): the wide bottom of the tree --
// millions of two- and three-leaf nodes over six or seven levels -- costs one level.
template <int kSahBlock>
__global__ void __launch_bounds__(kSahBlock) k_sah_level(const SahTask* __restrict__ queue_in, const uint32_t* __restrict__ n_in,
                                                         uint32_t* idx_a /* read by the level's nodes */, uint32_t* idx_b /* written */,
                                                         SahTask* __restrict__ queue_out, uint32_t* __restrict__ n_out, int n_leaves,
                                                         const float4* __restrict__ leaf_lo, const float4* __restrict__ leaf_hi,
                                                         int2* __restrict__ children, int* __restrict__ parent, int force_halve) {
  if (blockIdx.x >= *n_in) return;
  constexpr int kLocalLeaves = 64;
  SahTask t = queue_in[blockIdx.x];
  const bool local = kSahBlock == 64 && t.e - t.b <= (uint32_t)kLocalLeaves;
  const int tid = threadIdx.x;
  __shared__ float s_red[6][kSahBlock / 64];
  __shared__ float s_clo[3], s_scale[3];
  __shared__ int s_box[3][kSahBins][6];      // ordered-int lo xyz, hi xyz
  __shared__ uint32_t s_count[3][kSahBins];
  __shared__ SahSplit s_split;
  __shared__ uint32_t s_wave_sum[kSahBlock / 64], s_done[2];
  __shared__ SahTask s_stack[kSahBlock == 64 ? kLocalLeaves : 1];   // bit 31 of .node: the task reads idx_b (its parent wrote there)
  __shared__ int s_sp;
  if (tid == 0) s_sp = 0;
  bool flip = false;
  for (;;) {
    const uint32_t* idx_in = flip ? idx_b : idx_a;
    uint32_t* idx_out = flip ? idx_a : idx_b;
    const uint32_t cnt = t.e - t.b;
    uint32_t mid = t.b + cnt / 2;
    bool found = false;
    if (cnt > 2 && !force_halve) {
      // ---- centroid bounds ----
      sah_reset_bins(&s_box[0][0][0], &s_count[0][0], tid, kSahBlock);
      float l, h;
      sah_block_centroid_bounds<kSahBlock>(t.b, t.e, idx_in, leaf_lo, leaf_hi, s_red, l, h);
      if (tid < 3) {
        s_clo[tid] = l;
        s_scale[tid] = h - l > 0.0f ? (float)kSahBins / (h - l) : 0.0f;
      }
      __syncthreads();
      // ---- binning ----
      for (uint32_t i = t.b + tid; i < t.e; i += kSahBlock) {
        const uint32_t p = idx_in[i];
        sah_bin_leaf(leaf_lo[p], leaf_hi[p], s_clo, s_scale, &s_box[0][0][0], &s_count[0][0]);
      }
      __syncthreads();
      if (tid == 0) s_split = sah_pick_split(&s_box[0][0][0], &s_count[0][0], s_scale);
      __syncthreads();
      found = s_split.axis >= 0 && s_split.n_left > 0 && s_split.n_left < cnt;
    }
    if (found) {
      mid = t.b + s_split.n_left;
      sah_scatter<kSahBlock>(t.b, t.e, t.b, mid, s_split.axis, s_split.bin, s_clo[s_split.axis], s_scale[s_split.axis], 0u, 0u, idx_in, idx_out, leaf_lo, leaf_hi, s_wave_sum, s_done);
    } else {
      for (uint32_t i = t.b + tid; i < t.e; i += kSahBlock) idx_out[i] = idx_in[i];   // two leaves, or every centroid in one place: halve the range as it stands
      __syncthreads();
    }
    if (!local) {
      if (tid == 0) sah_emit_children(t, mid, idx_out, n_leaves, children, parent, queue_out, n_out);
      return;
    }
    // ---- this wave goes on with the children ----
    if (tid == 0)
      sah_link_children(t, mid, idx_out, n_leaves, children, parent, [stack = &s_stack[0], sp = &s_sp, flip](const SahTask& child) {
        stack[(*sp)++] = SahTask{child.b, child.e, child.node | (flip ? 0 : (int)0x80000000)};   // the child reads what this node wrote
      });
    __syncthreads();
    if (s_sp == 0) return;
    t = s_stack[s_sp - 1];
    __syncthreads();
    if (tid == 0) --s_sp;
    flip = (t.node & (int)0x80000000) != 0;
    t.node &= 0x7FFFFFFF;
    __syncthreads();
  }
}
// ---- the top levels: long ranges, several blocks per node ("chunks" of kSahChunk elements) ----
// A level whose mean range is long would leave a handful of blocks looping over millions of elements (level 0 of 3.6 M
// leaves: 70 ms in one block).  Here every pass of the level runs over (node, chunk) pairs: centroid bounds and bins are
// combined per node with global atomics on ordered ints (min / max / counts: the result does not depend on the order), the
// split is picked by one thread per node with the same routine, lefts are counted per chunk, and every chunk scatters
// its elements behind those of the chunks before it -- the stable partition of the one-block version, hence the same tree.
constexpr int kSahMaxSplitLevels = 256;   // levels of SAH splits before the rest of the tree is built by halving ranges
constexpr uint32_t kSahChunk = 4096;
constexpr uint32_t kSahWideMean = 16384;   // levels whose mean range is at least this long take the several-blocks-per-node path
constexpr int kSahWideBlock = 1024;
struct SahWideNode {
  int bounds[6];                       // ordered-int centroid lo xyz, hi xyz
  int box[3 * kSahBins * 6];
  uint32_t count[3 * kSahBins];
  SahSplit split;
  uint32_t found;
  uint32_t chunk_base;                 // number of the node's first chunk in the level
};
// The preamble of the per-chunk kernels: block -> node of the level, chunk of the node and the chunk's elements [begin, end); false
// when the block is beyond the level's chunks
struct SahChunk {
  uint32_t node, chunk, begin, end;
  SahTask t;
};
__device__ __forceinline__ bool sah_chunk_of_block(const SahTask* __restrict__ queue_in, const uint32_t* __restrict__ n_in, const uint32_t* __restrict__ total_chunks,
                                                   const SahWideNode* __restrict__ wide, SahChunk& c) {
  if (blockIdx.x >= *total_chunks) return false;
  uint32_t lo = 0, hi = *n_in - 1;
  while (lo < hi) {   // last node whose first chunk is <= block
    const uint32_t m = (lo + hi + 1) >> 1;
    if (wide[m].chunk_base <= blockIdx.x) lo = m; else hi = m - 1;
  }
  c.node = lo;
  c.chunk = blockIdx.x - wide[lo].chunk_base;
  c.t = queue_in[c.node];
  c.begin = c.t.b + c.chunk * kSahChunk;
  c.end = min(c.t.e, c.begin + kSahChunk);
  return true;
}
__global__ void __launch_bounds__(1024) k_wide_plan(const SahTask* __restrict__ queue_in, const uint32_t* __restrict__ n_in, SahWideNode* __restrict__ wide,
                                                    uint32_t* __restrict__ total_chunks) {
  const uint32_t n_nodes = *n_in;
  for (uint32_t i = threadIdx.x; i < n_nodes; i += blockDim.x) {
    SahWideNode& w = wide[i];
    for (int k = 0; k < 3; ++k) { w.bounds[k] = float_to_ordered(INFINITY); w.bounds[3 + k] = float_to_ordered(-INFINITY); }
    sah_reset_bins(w.box, w.count, 0, 1);
    w.split = SahSplit{-1, -1, 0u}; w.found = 0;
  }
  if (threadIdx.x == 0) {
    uint32_t acc = 0;
    for (uint32_t i = 0; i < n_nodes; ++i) { wide[i].chunk_base = acc; acc += (queue_in[i].e - queue_in[i].b + kSahChunk - 1) / kSahChunk; }
    *total_chunks = acc;
  }
}
__global__ void __launch_bounds__(kSahWideBlock) k_wide_bounds(const SahTask* __restrict__ queue_in, const uint32_t* __restrict__ n_in,
                                                               const uint32_t* __restrict__ total_chunks, SahWideNode* __restrict__ wide,
                                                               const uint32_t* __restrict__ idx_in, const float4* __restrict__ leaf_lo,
                                                               const float4* __restrict__ leaf_hi) {
  SahChunk c;
  if (!sah_chunk_of_block(queue_in, n_in, total_chunks, wide, c) || c.t.e - c.t.b <= 2) return;
  __shared__ float s_red[6][kSahWideBlock / 64];
  const int tid = threadIdx.x;
  float l, h;
  sah_block_centroid_bounds<kSahWideBlock>(c.begin, c.end, idx_in, leaf_lo, leaf_hi, s_red, l, h);
  if (tid < 3) {
    atomicMin(&wide[c.node].bounds[tid], float_to_ordered(l));
    atomicMax(&wide[c.node].bounds[3 + tid], float_to_ordered(h));
  }
}
__device__ __forceinline__ void sah_wide_scale(const SahWideNode& w, float clo[3], float scale[3]) {
  for (int a = 0; a < 3; ++a) {
    const float l = ordered_to_float(w.bounds[a]), h = ordered_to_float(w.bounds[3 + a]);
    clo[a] = l;
    scale[a] = h - l > 0.0f ? (float)kSahBins / (h - l) : 0.0f;
  }
}
__global__ void __launch_bounds__(kSahWideBlock) k_wide_bin(const SahTask* __restrict__ queue_in, const uint32_t* __restrict__ n_in,
                                                            const uint32_t* __restrict__ total_chunks, SahWideNode* __restrict__ wide,
                                                            const uint32_t* __restrict__ idx_in, const float4* __restrict__ leaf_lo,
                                                            const float4* __restrict__ leaf_hi) {
  SahChunk c;
  if (!sah_chunk_of_block(queue_in, n_in, total_chunks, wide, c) || c.t.e - c.t.b <= 2) return;
  __shared__ int s_box[3 * kSahBins * 6];
  __shared__ uint32_t s_count[3 * kSahBins];
  const int tid = threadIdx.x;
  sah_reset_bins(s_box, s_count, tid, kSahWideBlock);
  float clo[3], scale[3];
  sah_wide_scale(wide[c.node], clo, scale);
  __syncthreads();
  for (uint32_t i = c.begin + tid; i < c.end; i += kSahWideBlock) {
    const uint32_t p = idx_in[i];
    sah_bin_leaf(leaf_lo[p], leaf_hi[p], clo, scale, s_box, s_count);
  }
  __syncthreads();
  for (int i = tid; i < 3 * kSahBins; i += kSahWideBlock) {
    if (s_count[i] == 0) continue;
    atomicAdd(&wide[c.node].count[i], s_count[i]);
    for (int d = 0; d < 3; ++d) { atomicMin(&wide[c.node].box[i * 6 + d], s_box[i * 6 + d]); atomicMax(&wide[c.node].box[i * 6 + 3 + d], s_box[i * 6 + 3 + d]); }
  }
}
__global__ void __launch_bounds__(64) k_wide_pick(const SahTask* __restrict__ queue_in, const uint32_t* __restrict__ n_in, SahWideNode* __restrict__ wide) {
  const uint32_t node = blockIdx.x * blockDim.x + threadIdx.x;
  if (node >= *n_in) return;
  const SahTask t = queue_in[node];
  const uint32_t cnt = t.e - t.b;
  if (cnt <= 2) return;
  float clo[3], scale[3];
  sah_wide_scale(wide[node], clo, scale);
  const SahSplit s = sah_pick_split(wide[node].box, wide[node].count, scale);
  wide[node].split = s;
  wide[node].found = (s.axis >= 0 && s.n_left > 0 && s.n_left < cnt) ? 1u : 0u;
}
__global__ void __launch_bounds__(kSahWideBlock) k_wide_count(const SahTask* __restrict__ queue_in, const uint32_t* __restrict__ n_in,
                                                              const uint32_t* __restrict__ total_chunks, const SahWideNode* __restrict__ wide,
                                                              const uint32_t* __restrict__ idx_in, const float4* __restrict__ leaf_lo,
                                                              const float4* __restrict__ leaf_hi, uint32_t* __restrict__ chunk_left) {
  SahChunk c;
  if (!sah_chunk_of_block(queue_in, n_in, total_chunks, wide, c)) return;
  const SahWideNode& w = wide[c.node];
  if (!w.found) return;
  __shared__ uint32_t s_sum[kSahWideBlock / 64];
  float clo[3], scale[3];
  sah_wide_scale(w, clo, scale);
  const int axis = w.split.axis, bin = w.split.bin, tid = threadIdx.x;
  uint32_t mine = 0;
  for (uint32_t i = c.begin + tid; i < c.end; i += kSahWideBlock) {
    const uint32_t p = idx_in[i];
    mine += sah_bin_of(box_centroid(leaf_lo[p], leaf_hi[p], axis), clo[axis], scale[axis]) <= bin ? 1u : 0u;
  }
  const uint32_t total = sah_block_sum<kSahWideBlock>(mine, s_sum);
  if (tid == 0) chunk_left[blockIdx.x] = total;
}
__global__ void __launch_bounds__(kSahWideBlock) k_wide_scatter(const SahTask* __restrict__ queue_in, const uint32_t* __restrict__ n_in,
                                                                const uint32_t* __restrict__ total_chunks, const SahWideNode* __restrict__ wide,
                                                                const uint32_t* __restrict__ chunk_left, const uint32_t* __restrict__ idx_in,
                                                                uint32_t* __restrict__ idx_out, const float4* __restrict__ leaf_lo,
                                                                const float4* __restrict__ leaf_hi) {
  SahChunk c;
  if (!sah_chunk_of_block(queue_in, n_in, total_chunks, wide, c)) return;
  const SahWideNode& w = wide[c.node];
  const int tid = threadIdx.x;
  if (!w.found) {   // the range stays as it is
    for (uint32_t i = c.begin + tid; i < c.end; i += kSahWideBlock) idx_out[i] = idx_in[i];
    return;
  }
  __shared__ uint32_t s_sum[kSahWideBlock / 64], s_wave_sum[kSahWideBlock / 64], s_done[2], s_before;
  // lefts in the chunks of this node before this one
  uint32_t mine = 0;
  for (uint32_t k = tid; k < c.chunk; k += kSahWideBlock) mine += chunk_left[w.chunk_base + k];
  const uint32_t total = sah_block_sum<kSahWideBlock>(mine, s_sum);
  if (tid == 0) s_before = total;
  __syncthreads();
  const uint32_t left_before = s_before, right_before = c.chunk * kSahChunk - left_before;
  float clo[3], scale[3];
  sah_wide_scale(w, clo, scale);
  sah_scatter<kSahWideBlock>(c.begin, c.end, c.t.b, c.t.b + w.split.n_left, w.split.axis, w.split.bin, clo[w.split.axis], scale[w.split.axis], left_before, right_before, idx_in, idx_out, leaf_lo,
                             leaf_hi, s_wave_sum, s_done);
}
__global__ void __launch_bounds__(64) k_wide_children(const SahTask* __restrict__ queue_in, const uint32_t* __restrict__ n_in,
                                                      const SahWideNode* __restrict__ wide, const uint32_t* __restrict__ idx_out, int n_leaves,
                                                      int2* __restrict__ children, int* __restrict__ parent, SahTask* __restrict__ queue_out,
                                                      uint32_t* __restrict__ n_out) {
  const uint32_t node = blockIdx.x * blockDim.x + threadIdx.x;
  if (node >= *n_in) return;
  const SahTask t = queue_in[node];
  const uint32_t mid = wide[node].found ? t.b + wide[node].split.n_left : t.b + (t.e - t.b) / 2;
  sah_emit_children(t, mid, idx_out, n_leaves, children, parent, queue_out, n_out);
}

__global__ void k_sah_init(uint32_t n, uint32_t* __restrict__ idx, SahTask* __restrict__ queue, uint32_t* __restrict__ counts, int* __restrict__ parent) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) idx[i] = i;
  if (i == 0) {
    queue[0] = SahTask{0u, n, 0};
    counts[0] = 1;
    counts[1] = 0;
    parent[0] = -1;
  }
}

// Binned SAH, level by level; the leaf boxes are the node_lo / node_hi slots (n-1)+j of the build.
hipError_t build_sah_levels(hipStream_t st, uint32_t n, const float4* leaf_lo, const float4* leaf_hi, int2* children, int* parent) {
  DeviceBuffer<uint32_t> idx_a, idx_b, counts, total_chunks, chunk_left;
  DeviceBuffer<SahWideNode> wide;
  DeviceBuffer<SahTask> queue_a, queue_b;
  GLZ_TRY(alloc_each(n, idx_a, idx_b));
  GLZ_TRY(alloc_each((size_t)n / 2 + 2, queue_a, queue_b));
  GLZ_TRY(counts.alloc(2));
  GLZ_TRY(total_chunks.alloc(1));
  GLZ_TRY(wide.alloc((size_t)n / kSahWideMean + 2));
  GLZ_TRY(chunk_left.alloc((size_t)n / kSahWideMean + (size_t)n / kSahChunk + 4));
  GLZ_TRY(launch(k_sah_init, dim3((n + 255) / 256), dim3(256), st, n, idx_a.ptr, queue_a.ptr, counts.ptr, parent));
  uint32_t active = 1;
  uint32_t *idx_in = idx_a.ptr, *idx_out = idx_b.ptr;
  SahTask *q_in = queue_a.ptr, *q_out = queue_b.ptr;
  for (int level = 0, in = 0; active > 0; ++level, in ^= 1) {
    if (level > kSahMaxSplitLevels + 64) return hipErrorUnknown;   // cannot happen: halving ends after 32 levels
    // by the mean range of the level: several blocks per node while the ranges are long, then one block per node --
    // many threads for a long range (it is one block's loop), one wave for the wide bottom levels (its barriers cost nothing)
    // A tree this deep means input that defeats the binning level after level (a geometric progression of scales); the
    // remaining ranges are halved as they stand so that the depth stays bounded.
    const int force_halve = level >= kSahMaxSplitLevels ? 1 : 0;
    const uint32_t mean = n / active;
    uint32_t *n_in = counts.ptr + in, *n_out = counts.ptr + (in ^ 1);
    if (mean >= kSahWideMean && !force_halve) {
      const uint32_t max_chunks = active + n / kSahChunk + 1;
      const dim3 gc(max_chunks), gn((active + 63) / 64), wb(kSahWideBlock);
      GLZ_TRY(launch(k_wide_plan, dim3(1), dim3(1024), st, q_in, n_in, wide.ptr, total_chunks.ptr));
      GLZ_TRY(launch(k_wide_bounds, gc, wb, st, q_in, n_in, total_chunks.ptr, wide.ptr, idx_in, leaf_lo, leaf_hi));
      GLZ_TRY(launch(k_wide_bin, gc, wb, st, q_in, n_in, total_chunks.ptr, wide.ptr, idx_in, leaf_lo, leaf_hi));
      GLZ_TRY(launch(k_wide_pick, gn, dim3(64), st, q_in, n_in, wide.ptr));
      GLZ_TRY(launch(k_wide_count, gc, wb, st, q_in, n_in, total_chunks.ptr, wide.ptr, idx_in, leaf_lo, leaf_hi, chunk_left.ptr));
      GLZ_TRY(launch(k_wide_scatter, gc, wb, st, q_in, n_in, total_chunks.ptr, wide.ptr, chunk_left.ptr, idx_in, idx_out, leaf_lo, leaf_hi));
      GLZ_TRY(launch(k_wide_children, gn, dim3(64), st, q_in, n_in, wide.ptr, idx_out, (int)n, children, parent, q_out, n_out));
    } else {
      const auto one_block_per_node = [&](auto kernel, uint32_t block) {
        return launch(kernel, dim3(active), dim3(block), st, q_in, n_in, idx_in, idx_out, q_out, n_out, (int)n, leaf_lo, leaf_hi, children, parent, force_halve);
      };
      GLZ_TRY(mean >= 4096 ? one_block_per_node(k_sah_level<1024>, 1024) : mean >= 128 ? one_block_per_node(k_sah_level<256>, 256) : one_block_per_node(k_sah_level<64>, 64));
    }
    GLZ_TRY(hipMemcpyAsync(&active, n_out, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    GLZ_TRY(hipMemsetAsync(n_in, 0, sizeof(uint32_t), st));   // this level's input counter is the output counter of the level after next
    GLZ_TRY(hipStreamSynchronize(st));
    std::swap(idx_in, idx_out);
    std::swap(q_in, q_out);
  }
  return hipSuccess;
}

}  // namespace glz
