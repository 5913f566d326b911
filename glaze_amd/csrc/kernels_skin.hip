// k_skin: linear-blend skinning on the device (skin.h holds the rule, include/glaze_abi.h the specification); k_skin_dq, further down:
// dual-quaternion blending, for the skins set to that mode.
//
// A streaming kernel, bound by memory: per vertex 32 bytes of bind pose, 8 of joints and 16 of weights come in and 32 go out (88), all in
// whole dwordx4 / dwordx2 accesses of consecutive lanes; the arithmetic (66 multiplies, 51 adds) hides behind them.  One thread per vertex,
// a grid-stride loop over a grid that fills the chip once, so a block stages the bone table once for all the vertices it handles.
// STAGED: the table (three float4 rows a bone) fits kSkinLdsBones and is copied to LDS, whose reads (ds_read_b128) stay off the
// vector-memory path; otherwise the rows are read from memory (global_load_dwordx4).  One instantiation per address space, chosen at
// launch (k_shade's pattern): no access is FLAT.
// Nothing depends on the first vertex: `out` is a float4 pointer to that vertex (32-byte vertices: any vertex index is 16-byte aligned),
// and bind, joints and weights are the skin's own arrays, indexed from 0.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "kernels.h"
#include "skin.h"

namespace glz {

constexpr uint32_t kSkinBlock = 256;
// blocks the grid is capped at: eight 256-thread blocks on each of 256 compute units
constexpr uint32_t kSkinMaxBlocks = 2048;

template <class T>
__device__ __forceinline__ const T* in_memory(const T* p) { return (const T*)(const __attribute__((address_space(1))) T*)p; }

template <bool STAGED>
__global__ void __launch_bounds__(kSkinBlock) k_skin(const float4* __restrict__ bind, const uint2* __restrict__ joints, const float4* __restrict__ weights, uint32_t n,
                                                     const float4* __restrict__ bones, uint32_t n_bones, float4* __restrict__ out) {
  __shared__ float4 s_bones[STAGED ? kSkinLdsBones * post::kSkinBoneRows : 1];
  if (STAGED) {
    for (uint32_t k = threadIdx.x; k < post::kSkinBoneRows * n_bones; k += kSkinBlock) s_bones[k] = bones[k];
    __syncthreads();
  }
  for (size_t i = (size_t)blockIdx.x * kSkinBlock + threadIdx.x; i < n; i += (size_t)gridDim.x * kSkinBlock) {
    float4 v0 = bind[2 * i], v1 = bind[2 * i + 1];
    const uint2 jj = joints[i];
    const float4 w = weights[i];
    const uint32_t j[4] = {jj.x & 0xFFFFu, jj.x >> 16, jj.y & 0xFFFFu, jj.y >> 16};
    if (STAGED) post::skin_vertex(static_cast<const float4*>(s_bones), j, w, v0, v1);
    else post::skin_vertex(in_memory(bones), j, w, v0, v1);
    out[2 * i] = v0;
    out[2 * i + 1] = v1;
  }
}

// k_skin_dq: k_skin's sibling for a skin in dual-quaternion mode (skin.h skin_vertex_dq).  The same grid, the same loads and stores of
// the same 88 bytes a vertex; the table is two float4 a bone (post::pack_bone_dq), 8 KB of LDS at kSkinLdsBones.  The arithmetic is about
// three times k_skin's, with one correctly rounded square root and one division a vertex.
template <bool STAGED>
__global__ void __launch_bounds__(kSkinBlock) k_skin_dq(const float4* __restrict__ bind, const uint2* __restrict__ joints, const float4* __restrict__ weights, uint32_t n,
                                                        const float4* __restrict__ bones, uint32_t n_bones, float4* __restrict__ out) {
  __shared__ float4 s_bones[STAGED ? kSkinLdsBones * post::kSkinDqBoneRows : 1];
  if (STAGED) {
    for (uint32_t k = threadIdx.x; k < post::kSkinDqBoneRows * n_bones; k += kSkinBlock) s_bones[k] = bones[k];
    __syncthreads();
  }
  for (size_t i = (size_t)blockIdx.x * kSkinBlock + threadIdx.x; i < n; i += (size_t)gridDim.x * kSkinBlock) {
    float4 v0 = bind[2 * i], v1 = bind[2 * i + 1];
    const uint2 jj = joints[i];
    const float4 w = weights[i];
    const uint32_t j[4] = {jj.x & 0xFFFFu, jj.x >> 16, jj.y & 0xFFFFu, jj.y >> 16};
    if (STAGED) post::skin_vertex_dq(static_cast<const float4*>(s_bones), j, w, v0, v1);
    else post::skin_vertex_dq(in_memory(bones), j, w, v0, v1);
    out[2 * i] = v0;
    out[2 * i + 1] = v1;
  }
}

static uint32_t skin_blocks(uint32_t n) { return (uint32_t)std::min<uint64_t>(((uint64_t)n + kSkinBlock - 1) / kSkinBlock, kSkinMaxBlocks); }

hipError_t launch_skin(hipStream_t st, const float4* bind, const uint2* joints, const float4* weights, uint32_t n, const float4* bones, uint32_t n_bones, float4* out) {
  if (n == 0) return hipSuccess;
  const uint32_t blocks = skin_blocks(n);
  if (n_bones <= kSkinLdsBones) hipLaunchKernelGGL(k_skin<true>, dim3(blocks), dim3(kSkinBlock), 0, st, bind, joints, weights, n, bones, n_bones, out);
  else hipLaunchKernelGGL(k_skin<false>, dim3(blocks), dim3(kSkinBlock), 0, st, bind, joints, weights, n, bones, n_bones, out);
  return hipGetLastError();
}

hipError_t launch_skin_dq(hipStream_t st, const float4* bind, const uint2* joints, const float4* weights, uint32_t n, const float4* bones, uint32_t n_bones, float4* out) {
  if (n == 0) return hipSuccess;
  const uint32_t blocks = skin_blocks(n);
  if (n_bones <= kSkinLdsBones) hipLaunchKernelGGL(k_skin_dq<true>, dim3(blocks), dim3(kSkinBlock), 0, st, bind, joints, weights, n, bones, n_bones, out);
  else hipLaunchKernelGGL(k_skin_dq<false>, dim3(blocks), dim3(kSkinBlock), 0, st, bind, joints, weights, n, bones, n_bones, out);
  return hipGetLastError();
}

}  // namespace glz
