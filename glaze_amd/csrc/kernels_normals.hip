// k_face_vectors, k_vertex_normals: shading normals recomputed from the positions the device holds (normals.h holds the rule and the
// layout, include/glaze_abi.h the specification).
//
// TWO kernels in stream order, not one: a single pass would have one thread read a neighbour's (p.xyz, n.x) float4 while that neighbour's
// own thread stores it.  Here k_face_vectors reads positions and writes a buffer the set owns; k_vertex_normals reads that buffer and its
// OWN vertex, and writes its own vertex: no word is read by one thread and written by another within a kernel.
//
// k_face_vectors: one thread per face, k_skin's grid-stride shape and block cap.  Per face 12 bytes of indices come in (consecutive
// lanes, consecutive dwords), three float4 are gathered -- the position and the first normal word of a corner, one 16-byte-aligned
// dwordx4 each -- and one float4 goes out, consecutive lanes, consecutive float4.
//
// k_vertex_normals: a gather, not a scatter (k_morph's structure): add_normals has made a row of face numbers per vertex (sliced ELLPACK,
// one slice a wavefront), so a thread owns its vertex, walks its row in ascending face order -- the order the rule fixes -- and stores
// once.  No atomics.  A step of a slice is 64 consecutive uint32, one 256-byte access of the wave, then the 16-byte face vectors they
// name; the walk takes eight steps at a time, the eight face numbers first and then the eight face vectors, so that a wave waits for two
// rounds of loads a chunk and not for two dependent loads a step (EXPERIMENTS.md has what that bought).  The step loop's bound is the
// slice's width taken through readfirstlane: a scalar, so the loop is uniform by construction; a lane past its own count is masked for
// the step's additions (its loads name the slice's zero padding, face 0), and a slice whose counts all equal its width runs unmasked.
// A vertex with no face stores nothing.  Per vertex: 4 bytes of count, 4 + 16 an entry of its row, 32 in, and 32 out of which 12 are new.
// Every access is to the global address space: none is FLAT.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "kernels.h"
#include "normals.h"

namespace glz {

constexpr uint32_t kNormalBlock = 256;
// blocks the grid is capped at: eight 256-thread blocks on each of 256 compute units (k_skin's cap)
constexpr uint32_t kNormalMaxBlocks = 2048;
static_assert(kNormalBlock % post::kNormalSlice == 0, "a wave's 64 vertices are one slice: blocks and the grid's stride are whole slices");

template <class T>
__device__ __forceinline__ const T* in_memory(const T* p) { return (const T*)(const __attribute__((address_space(1))) T*)p; }

__global__ void __launch_bounds__(kNormalBlock) k_face_vectors(const float4* __restrict__ vertices, const uint32_t* __restrict__ faces, uint32_t n_faces,
                                                               float4* __restrict__ face_vectors) {
  for (size_t f = (size_t)blockIdx.x * kNormalBlock + threadIdx.x; f < n_faces; f += (size_t)gridDim.x * kNormalBlock) {
    const uint32_t i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
    face_vectors[f] = post::face_vector(vertices[2 * (size_t)i0], vertices[2 * (size_t)i1], vertices[2 * (size_t)i2]);
  }
}

// in / out: the set's first vertex, in the scene's vertex buffer both (the same pointer), or out a scratch buffer (the timing hook): a
// thread reads and writes its own vertex alone, so the two may be one
__global__ void __launch_bounds__(kNormalBlock) k_vertex_normals(const float4* in, const uint32_t* __restrict__ counts, const uint2* __restrict__ slices,
                                                                 const uint32_t* __restrict__ rows, const float4* __restrict__ face_vectors, uint32_t n, float4* out) {
  for (size_t i = (size_t)blockIdx.x * kNormalBlock + threadIdx.x; i < n; i += (size_t)gridDim.x * kNormalBlock) {
    // i's wave holds slice i / 64 (all of its active lanes do), lane i % 64 its own row
    const uint2 slice = slices[i / post::kNormalSlice];
    const uint32_t first = __builtin_amdgcn_readfirstlane(slice.x), width = __builtin_amdgcn_readfirstlane(slice.y);
    const uint32_t* lane_row = in_memory(rows) + first + (uint32_t)(i % post::kNormalSlice);
    const uint32_t count = counts[i];
    // A slice whose rows are all as long as it is wide (a closed regular grid makes every slice so) has no padding and masks no lane:
    // with the count a scalar too, the loop's steps carry no EXEC mask and the loads of the steps the compiler unrolls issue together.
    const float4 normal = __builtin_amdgcn_ballot_w64(count != width) == 0 ? post::vertex_normal(lane_row, width, width, in_memory(face_vectors))
                                                                           : post::vertex_normal(lane_row, width, count, in_memory(face_vectors));
    if (count != 0) {
      float4 v0 = in[2 * i], v1 = in[2 * i + 1];
      v0.w = normal.x;
      v1.x = normal.y;
      v1.y = normal.z;
      out[2 * i] = v0;
      out[2 * i + 1] = v1;
    }
  }
}

static uint32_t normal_blocks(uint32_t n) { return (uint32_t)std::min<uint64_t>(((uint64_t)n + kNormalBlock - 1) / kNormalBlock, kNormalMaxBlocks); }

hipError_t launch_face_vectors(hipStream_t st, const float4* vertices, const NormalArgs& a, float4* face_vectors) {
  if (a.n_faces == 0) return hipSuccess;
  hipLaunchKernelGGL(k_face_vectors, dim3(normal_blocks(a.n_faces)), dim3(kNormalBlock), 0, st, vertices, a.faces, a.n_faces, face_vectors);
  return hipGetLastError();
}

hipError_t launch_vertex_normals(hipStream_t st, const float4* in, const NormalArgs& a, const float4* face_vectors, float4* out) {
  if (a.n == 0 || a.n_faces == 0) return hipSuccess;
  hipLaunchKernelGGL(k_vertex_normals, dim3(normal_blocks(a.n)), dim3(kNormalBlock), 0, st, in, a.counts, a.slices, a.rows, face_vectors, a.n, out);
  return hipGetLastError();
}

}  // namespace glz
