// k_morph, k_morph_skin: morph targets on the device (morph.h holds the rule and the layout, include/glaze_abi.h the specification).
//
// A gather, not a scatter: add_morph has transposed the per-target lists into rows a vertex (sliced ELLPACK, one slice a wavefront), so a
// thread owns its vertex, walks its own row in ascending target order -- the order the rule fixes -- and stores once.  No atomics.
// One thread per vertex, one wave per slice, 256-thread blocks, a grid-stride loop over a grid that fills the chip once (k_skin's cap), so
// a block stages its tables once for all the vertices it handles.
//
// AN ENTRY is 32 bytes, two float4: (d_position.xyz, target index) and (d_normal.xyz, unused).  The two halves live in two planes of 64
// float4 a step, so a wave's access to a step is two loads of consecutive float4 over one whole kilobyte each, whatever lanes are active
// (global_load_dwordx4, and dwordx3 for the normal plane, whose fourth word the compiler sees is unused).  What that packing costs: 4 of the 32 bytes carry nothing (the second spare word), 12.5 %; a 28-byte entry would save them and
// lose the dwordx4 access.  Padding -- steps past a lane's own count, up to its slice's width -- is neither read nor computed: the lane is
// masked off for the step (its cache lines still move where a neighbour in the same 64 bytes is active).
// Per vertex, besides its entries: 32 bytes of base in, 32 out, 4 of row length; per slice 8 bytes (offset, width), one address for the
// whole wave.  The step loop's bound is the slice's width taken through readfirstlane: a scalar, so the loop is uniform by construction.
//
// STAGED: the weight table (one float a target) fits kMorphLdsTargets and is copied to LDS, whose reads (ds_read_b32) stay off the
// vector-memory path; otherwise the weights are read from memory (global_load_dword).  k_morph_skin stages the bone table by k_skin's own
// rule, independently: four instantiations, and four more of k_morph_skin_dq for skins in dual-quaternion mode.  One instantiation per
// address space, chosen at launch: no access is FLAT.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "kernels.h"
#include "morph.h"
#include "skin.h"

namespace glz {

constexpr uint32_t kMorphBlock = 256;
// blocks the grid is capped at: eight 256-thread blocks on each of 256 compute units (k_skin's cap)
constexpr uint32_t kMorphMaxBlocks = 2048;
static_assert(kMorphBlock % post::kMorphSlice == 0, "a wave's 64 vertices are one slice: blocks and the grid's stride are whole slices");

template <class T>
__device__ __forceinline__ const T* in_memory(const T* p) { return (const T*)(const __attribute__((address_space(1))) T*)p; }

// vertex i of the morph under its row: i's wave holds slice i / 64 (all of its active lanes do), lane i % 64 its own row
template <class Weights>
__device__ __forceinline__ void morph_row(size_t i, const uint32_t* __restrict__ counts, const uint2* __restrict__ slices, const float4* __restrict__ entries, Weights weights,
                                          float4& v0, float4& v1) {
  const uint2 slice = slices[i / post::kMorphSlice];
  const uint32_t first = __builtin_amdgcn_readfirstlane(slice.x), width = __builtin_amdgcn_readfirstlane(slice.y);
  const float4* lane_entries = in_memory(entries) + first + (uint32_t)(i % post::kMorphSlice);
  const uint32_t count = counts[i];
  // A slice whose rows are all as long as it is wide (dense targets make every slice so) has no padding and masks no lane: with the
  // count a scalar too, the loop's steps carry no EXEC mask and the compiler issues the loads of the steps it unrolls together.
  if (__builtin_amdgcn_ballot_w64(count != width) == 0) post::morph_vertex(lane_entries, width, width, weights, v0, v1);
  else post::morph_vertex(lane_entries, width, count, weights, v0, v1);
}

template <bool STAGED>
__global__ void __launch_bounds__(kMorphBlock) k_morph(const float4* __restrict__ base, const uint32_t* __restrict__ counts, const uint2* __restrict__ slices,
                                                       const float4* __restrict__ entries, uint32_t n, const float* __restrict__ weights, uint32_t n_targets,
                                                       float4* __restrict__ out) {
  __shared__ float s_weights[STAGED ? kMorphLdsTargets : 1];
  if (STAGED) {
    for (uint32_t k = threadIdx.x; k < n_targets; k += kMorphBlock) s_weights[k] = weights[k];
    __syncthreads();
  }
  for (size_t i = (size_t)blockIdx.x * kMorphBlock + threadIdx.x; i < n; i += (size_t)gridDim.x * kMorphBlock) {
    float4 v0 = base[2 * i], v1 = base[2 * i + 1];
    if (STAGED) morph_row(i, counts, slices, entries, static_cast<const float*>(s_weights), v0, v1);
    else morph_row(i, counts, slices, entries, in_memory(weights), v0, v1);
    out[2 * i] = v0;
    out[2 * i + 1] = v1;
  }
}

template <bool STAGED, bool BONES_STAGED>
__global__ void __launch_bounds__(kMorphBlock) k_morph_skin(const float4* __restrict__ bind, const uint32_t* __restrict__ counts, const uint2* __restrict__ slices,
                                                            const float4* __restrict__ entries, uint32_t n, const float* __restrict__ weights, uint32_t n_targets,
                                                            const uint2* __restrict__ joints, const float4* __restrict__ skin_weights,
                                                            const float4* __restrict__ bones, uint32_t n_bones, float4* __restrict__ out) {
  __shared__ float s_weights[STAGED ? kMorphLdsTargets : 1];
  __shared__ float4 s_bones[BONES_STAGED ? kSkinLdsBones * post::kSkinBoneRows : 1];
  if (STAGED)
    for (uint32_t k = threadIdx.x; k < n_targets; k += kMorphBlock) s_weights[k] = weights[k];
  if (BONES_STAGED)
    for (uint32_t k = threadIdx.x; k < post::kSkinBoneRows * n_bones; k += kMorphBlock) s_bones[k] = bones[k];
  if (STAGED || BONES_STAGED) __syncthreads();
  for (size_t i = (size_t)blockIdx.x * kMorphBlock + threadIdx.x; i < n; i += (size_t)gridDim.x * kMorphBlock) {
    float4 v0 = bind[2 * i], v1 = bind[2 * i + 1];
    const uint2 jj = joints[i];
    const float4 w = skin_weights[i];
    if (STAGED) morph_row(i, counts, slices, entries, static_cast<const float*>(s_weights), v0, v1);
    else morph_row(i, counts, slices, entries, in_memory(weights), v0, v1);
    const uint32_t j[4] = {jj.x & 0xFFFFu, jj.x >> 16, jj.y & 0xFFFFu, jj.y >> 16};
    if (BONES_STAGED) post::skin_vertex(static_cast<const float4*>(s_bones), j, w, v0, v1);
    else post::skin_vertex(in_memory(bones), j, w, v0, v1);
    out[2 * i] = v0;
    out[2 * i + 1] = v1;
  }
}

// k_morph_skin for a skin in dual-quaternion mode: the same morph walk, then skin_vertex_dq on the registers, one store.  The bone table is
// two float4 a bone (post::pack_bone_dq), staged by k_skin_dq's rule.
template <bool STAGED, bool BONES_STAGED>
__global__ void __launch_bounds__(kMorphBlock) k_morph_skin_dq(const float4* __restrict__ bind, const uint32_t* __restrict__ counts, const uint2* __restrict__ slices,
                                                               const float4* __restrict__ entries, uint32_t n, const float* __restrict__ weights, uint32_t n_targets,
                                                               const uint2* __restrict__ joints, const float4* __restrict__ skin_weights,
                                                               const float4* __restrict__ bones, uint32_t n_bones, float4* __restrict__ out) {
  __shared__ float s_weights[STAGED ? kMorphLdsTargets : 1];
  __shared__ float4 s_bones[BONES_STAGED ? kSkinLdsBones * post::kSkinDqBoneRows : 1];
  if (STAGED)
    for (uint32_t k = threadIdx.x; k < n_targets; k += kMorphBlock) s_weights[k] = weights[k];
  if (BONES_STAGED)
    for (uint32_t k = threadIdx.x; k < post::kSkinDqBoneRows * n_bones; k += kMorphBlock) s_bones[k] = bones[k];
  if (STAGED || BONES_STAGED) __syncthreads();
  for (size_t i = (size_t)blockIdx.x * kMorphBlock + threadIdx.x; i < n; i += (size_t)gridDim.x * kMorphBlock) {
    float4 v0 = bind[2 * i], v1 = bind[2 * i + 1];
    const uint2 jj = joints[i];
    const float4 w = skin_weights[i];
    if (STAGED) morph_row(i, counts, slices, entries, static_cast<const float*>(s_weights), v0, v1);
    else morph_row(i, counts, slices, entries, in_memory(weights), v0, v1);
    const uint32_t j[4] = {jj.x & 0xFFFFu, jj.x >> 16, jj.y & 0xFFFFu, jj.y >> 16};
    if (BONES_STAGED) post::skin_vertex_dq(static_cast<const float4*>(s_bones), j, w, v0, v1);
    else post::skin_vertex_dq(in_memory(bones), j, w, v0, v1);
    out[2 * i] = v0;
    out[2 * i + 1] = v1;
  }
}

static uint32_t morph_blocks(uint32_t n) { return (uint32_t)std::min<uint64_t>(((uint64_t)n + kMorphBlock - 1) / kMorphBlock, kMorphMaxBlocks); }

hipError_t launch_morph(hipStream_t st, const MorphArgs& m, float4* out) {
  if (m.n == 0) return hipSuccess;
  const dim3 grid(morph_blocks(m.n)), block(kMorphBlock);
  if (m.n_targets <= kMorphLdsTargets) hipLaunchKernelGGL(k_morph<true>, grid, block, 0, st, m.base, m.counts, m.slices, m.entries, m.n, m.weights, m.n_targets, out);
  else hipLaunchKernelGGL(k_morph<false>, grid, block, 0, st, m.base, m.counts, m.slices, m.entries, m.n, m.weights, m.n_targets, out);
  return hipGetLastError();
}

template <bool STAGED>
static void launch_morph_skin_as(hipStream_t st, const MorphArgs& m, const uint2* joints, const float4* skin_weights, const float4* bones, uint32_t n_bones, float4* out) {
  const dim3 grid(morph_blocks(m.n)), block(kMorphBlock);
  if (n_bones <= kSkinLdsBones)
    hipLaunchKernelGGL((k_morph_skin<STAGED, true>), grid, block, 0, st, m.base, m.counts, m.slices, m.entries, m.n, m.weights, m.n_targets, joints, skin_weights, bones, n_bones, out);
  else
    hipLaunchKernelGGL((k_morph_skin<STAGED, false>), grid, block, 0, st, m.base, m.counts, m.slices, m.entries, m.n, m.weights, m.n_targets, joints, skin_weights, bones, n_bones, out);
}

hipError_t launch_morph_skin(hipStream_t st, const MorphArgs& m, const uint2* joints, const float4* skin_weights, const float4* bones, uint32_t n_bones, float4* out) {
  if (m.n == 0) return hipSuccess;
  if (m.n_targets <= kMorphLdsTargets) launch_morph_skin_as<true>(st, m, joints, skin_weights, bones, n_bones, out);
  else launch_morph_skin_as<false>(st, m, joints, skin_weights, bones, n_bones, out);
  return hipGetLastError();
}

template <bool STAGED>
static void launch_morph_skin_dq_as(hipStream_t st, const MorphArgs& m, const uint2* joints, const float4* skin_weights, const float4* bones, uint32_t n_bones, float4* out) {
  const dim3 grid(morph_blocks(m.n)), block(kMorphBlock);
  if (n_bones <= kSkinLdsBones)
    hipLaunchKernelGGL((k_morph_skin_dq<STAGED, true>), grid, block, 0, st, m.base, m.counts, m.slices, m.entries, m.n, m.weights, m.n_targets, joints, skin_weights, bones, n_bones, out);
  else
    hipLaunchKernelGGL((k_morph_skin_dq<STAGED, false>), grid, block, 0, st, m.base, m.counts, m.slices, m.entries, m.n, m.weights, m.n_targets, joints, skin_weights, bones, n_bones, out);
}

hipError_t launch_morph_skin_dq(hipStream_t st, const MorphArgs& m, const uint2* joints, const float4* skin_weights, const float4* bones, uint32_t n_bones, float4* out) {
  if (m.n == 0) return hipSuccess;
  if (m.n_targets <= kMorphLdsTargets) launch_morph_skin_dq_as<true>(st, m, joints, skin_weights, bones, n_bones, out);
  else launch_morph_skin_dq_as<false>(st, m, joints, skin_weights, bones, n_bones, out);
  return hipGetLastError();
}

}  // namespace glz
