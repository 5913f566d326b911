// k_deform: the vertex deformers on the device -- morph targets (morph.h holds the rule and the layout), then skinning (skin.h holds the
// two rules: linear blend and dual quaternion); include/glaze_abi.h holds the specifications.  One kernel template, instantiated per
// combination that runs: a morph alone (the old k_morph), a skin alone (k_skin, k_skin_dq), or the morph and then the skin on the
// registers with one store (k_morph_skin, k_morph_skin_dq).
//
// A streaming kernel, bound by memory, all in whole dwordx4 / dwordx2 accesses of consecutive lanes.  One thread per vertex, 256-thread
// blocks, a grid-stride loop over a grid that fills the chip once, so a block stages its tables once for all the vertices it handles.
// Nothing depends on the first vertex: `out` is a float4 pointer to that vertex (32-byte vertices: any vertex index is 16-byte aligned),
// and base, joints and weights are the deformer's own arrays, indexed from 0.
//
// THE SKIN STEP: per vertex 32 bytes of bind pose, 8 of joints and 16 of weights come in and 32 go out (88); the linear rule's arithmetic
// (66 multiplies, 51 adds) hides behind them.  The dual-quaternion rule moves the same 88 bytes; its arithmetic is about three times the
// linear rule's, with one correctly rounded square root and one division a vertex.
// BONES_STAGED: the bone table (three float4 rows a bone, 12 KB at kSkinLdsBones; two a bone under the dual-quaternion rule,
// post::pack_bone_dq, 8 KB) fits kSkinLdsBones and is copied to LDS, whose reads (ds_read_b128) stay off the vector-memory path;
// otherwise the rows are read from memory (global_load_dwordx4).
//
// THE MORPH STEP is a gather, not a scatter: add_morph has transposed the per-target lists into rows a vertex (sliced ELLPACK, one slice
// a wavefront), so a thread owns its vertex, walks its own row in ascending target order -- the order the rule fixes -- and stores once.
// No atomics.  One wave per slice.
// AN ENTRY is 32 bytes, two float4: (d_position.xyz, target index) and (d_normal.xyz, unused).  The two halves live in two planes of 64
// float4 a step, so a wave's access to a step is two loads of consecutive float4 over one whole kilobyte each, whatever lanes are active
// (global_load_dwordx4, and dwordx3 for the normal plane, whose fourth word the compiler sees is unused).  What that packing costs: 4 of
// the 32 bytes carry nothing (the second spare word), 12.5 %; a 28-byte entry would save them and lose the dwordx4 access.  Padding --
// steps past a lane's own count, up to its slice's width -- is neither read nor computed: the lane is masked off for the step (its cache
// lines still move where a neighbour in the same 64 bytes is active).
// Per vertex, besides its entries: 32 bytes of base in, 32 out, 4 of row length; per slice 8 bytes (offset, width), one address for the
// whole wave.  The step loop's bound is the slice's width taken through readfirstlane: a scalar, so the loop is uniform by construction.
// kMorphStaged: the weight table (one float a target) fits kMorphLdsTargets and is copied to LDS, whose reads (ds_read_b32) stay off the
// vector-memory path; kMorphMemory: the weights are read from memory (global_load_dword).
//
// The two tables are staged independently, each by its own rule.  One instantiation per address space, chosen at launch (k_shade's
// pattern): no access is FLAT.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "kernels.h"
#include "morph.h"
#include "skin.h"

namespace glz {

constexpr uint32_t kDeformBlock = 256;
// blocks the grid is capped at: eight 256-thread blocks on each of 256 compute units
constexpr uint32_t kDeformMaxBlocks = 2048;
static_assert(kDeformBlock % post::kMorphSlice == 0, "a wave's 64 vertices are one slice: blocks and the grid's stride are whole slices");

enum { kMorphNone, kMorphStaged, kMorphMemory };   // the morph step: none, weights in LDS, weights from memory
enum { kSkinNone, kSkinLinear, kSkinDq };          // the skin step: none, skin_vertex, skin_vertex_dq

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

// the vertex under its four joints (four uint16 in one uint2) and weights, by the rule SKIN names
template <int SKIN>
__device__ __forceinline__ void skin_row(const float4* bones, uint2 jj, float4 w, float4& v0, float4& v1) {
  const uint32_t j[4] = {jj.x & 0xFFFFu, jj.x >> 16, jj.y & 0xFFFFu, jj.y >> 16};
  if constexpr (SKIN == kSkinDq) post::skin_vertex_dq(bones, j, w, v0, v1);
  else post::skin_vertex(bones, j, w, v0, v1);
}

// base: the morph's base or the skin's bind pose (with both, the bind pose IS the base).  The arguments of a step that is not compiled
// in are not read.
template <int MORPH, int SKIN, bool BONES_STAGED>
__global__ void __launch_bounds__(kDeformBlock) k_deform(const float4* __restrict__ base, const uint32_t* __restrict__ counts, const uint2* __restrict__ slices,
                                                         const float4* __restrict__ entries, uint32_t n, const float* __restrict__ weights, uint32_t n_targets,
                                                         const uint2* __restrict__ joints, const float4* __restrict__ skin_weights,
                                                         const float4* __restrict__ bones, uint32_t n_bones, float4* __restrict__ out) {
  static_assert(SKIN != kSkinNone || !BONES_STAGED, "no skin step, no bone table");
  constexpr uint32_t kBoneRows = SKIN == kSkinDq ? post::kSkinDqBoneRows : post::kSkinBoneRows;
  __shared__ float s_weights[MORPH == kMorphStaged ? kMorphLdsTargets : 1];
  __shared__ float4 s_bones[BONES_STAGED ? kSkinLdsBones * kBoneRows : 1];
  if (MORPH == kMorphStaged)
    for (uint32_t k = threadIdx.x; k < n_targets; k += kDeformBlock) s_weights[k] = weights[k];
  if (BONES_STAGED)
    for (uint32_t k = threadIdx.x; k < kBoneRows * n_bones; k += kDeformBlock) s_bones[k] = bones[k];
  if (MORPH == kMorphStaged || BONES_STAGED) __syncthreads();
  for (size_t i = (size_t)blockIdx.x * kDeformBlock + threadIdx.x; i < n; i += (size_t)gridDim.x * kDeformBlock) {
    float4 v0 = base[2 * i], v1 = base[2 * i + 1];
    uint2 jj;
    float4 w;
    if constexpr (SKIN != kSkinNone) {
      jj = joints[i];
      w = skin_weights[i];
    }
    if constexpr (MORPH == kMorphStaged) morph_row(i, counts, slices, entries, static_cast<const float*>(s_weights), v0, v1);
    if constexpr (MORPH == kMorphMemory) morph_row(i, counts, slices, entries, in_memory(weights), v0, v1);
    if constexpr (SKIN != kSkinNone && BONES_STAGED) skin_row<SKIN>(static_cast<const float4*>(s_bones), jj, w, v0, v1);
    if constexpr (SKIN != kSkinNone && !BONES_STAGED) skin_row<SKIN>(in_memory(bones), jj, w, v0, v1);
    out[2 * i] = v0;
    out[2 * i + 1] = v1;
  }
}

namespace {

struct Launch {
  hipStream_t st;
  const MorphArgs& m;
  const SkinArgs& s;
  const float4* base;
  uint32_t n;
  float4* out;
};

template <int MORPH, int SKIN, bool BONES_STAGED>
void launch_as(const Launch& l) {
  const uint32_t blocks = (uint32_t)std::min<uint64_t>(((uint64_t)l.n + kDeformBlock - 1) / kDeformBlock, kDeformMaxBlocks);
  hipLaunchKernelGGL((k_deform<MORPH, SKIN, BONES_STAGED>), dim3(blocks), dim3(kDeformBlock), 0, l.st, l.base, l.m.counts, l.m.slices, l.m.entries, l.n, l.m.weights,
                     l.m.n_targets, l.s.joints, l.s.weights, l.s.bones, l.s.n_bones, l.out);
}

// the skin step and the staging of its table, for a morph step that is chosen
template <int MORPH>
void launch_skin_step(const Launch& l, const SkinArgs* skin) {
  const bool staged = skin && skin->n_bones <= kSkinLdsBones;
  if (!skin) {
    if constexpr (MORPH != kMorphNone) launch_as<MORPH, kSkinNone, false>(l);
  } else if (skin->blend == GLZ_SKIN_DUAL_QUATERNION) {
    if (staged) launch_as<MORPH, kSkinDq, true>(l);
    else launch_as<MORPH, kSkinDq, false>(l);
  } else {
    if (staged) launch_as<MORPH, kSkinLinear, true>(l);
    else launch_as<MORPH, kSkinLinear, false>(l);
  }
}

}  // namespace

hipError_t launch_deform(hipStream_t st, const MorphArgs* morph, const SkinArgs* skin, float4* out) {
  if (!morph && !skin) return hipErrorInvalidValue;
  static const MorphArgs no_morph{};
  static const SkinArgs no_skin{};
  const Launch l{st, morph ? *morph : no_morph, skin ? *skin : no_skin, morph ? morph->base : skin->bind, morph ? morph->n : skin->n, out};
  if (l.n == 0) return hipSuccess;
  if (!morph) launch_skin_step<kMorphNone>(l, skin);
  else if (morph->n_targets <= kMorphLdsTargets) launch_skin_step<kMorphStaged>(l, skin);
  else launch_skin_step<kMorphMemory>(l, skin);
  return hipGetLastError();
}

}  // namespace glz
