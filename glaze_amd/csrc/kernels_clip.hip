// k_clip_bones: the bone tables (and morph weight tables) of playing skeletons, made on the device from keyframes -- THE CLIP RULE
// (include/glaze_abi.h holds the specification, clip.h the one definition the host reference compiles too).  What it writes is what
// k_deform reads: no bone and no weight crosses the bus.
//
// ONE BLOCK A PLAY, so a crowd is one launch.  256 threads: a level as wide as a crowd character's (tens of bones) is one pass of the
// stride loop, and the four waves share one compute unit's L1, which is what makes a workgroup barrier enough between the levels.
//   PHASE 1  lanes stride over the bones: the two keys of bone b are sampled (key data is bone-contiguous within a key: consecutive lanes
//            read consecutive floats) and its local matrix L[b] goes to the skeleton's world table.
//   PHASE 2  level after level (a level: the bones of one depth, clip_levels), lanes stride over the level's bones: W[b] = W[parent] o L[b]
//            (root o L[b] for a root) replaces L[b].  __syncthreads() between levels: a level reads what the one before it wrote.  The
//            product runs down the chain and is never regrouped, so how lanes and levels split the bones does not reach the bits.
//   PHASE 3  lanes stride over the bones: B[b] = W[b] o inverse_bind[b], as three rows (a linear skin) or through skin.h's bone_dual_quat
//            (GLZ_SKIN_DUAL_QUATERNION), into the bone table; lanes stride over the targets: the lerped weight track into the weight table.
// The world table is in MEMORY whatever the skeleton's size: 65 536 bones take the path one bone takes.  It is read and written through a
// plain pointer (not __restrict__, not const): the reads of phase 2 must be vector loads issued after the barrier.
// Every loop bound -- bone count, level count, level offsets, target count -- is the same for all lanes of the block and is taken
// through readfirstlane: scalars, so the loops are uniform by construction and the barrier in the level loop is reached by every wave.
#include <hip/hip_runtime.h>

#include "clip.h"
#include "kernels.h"
#include "skin.h"

namespace glz {

constexpr uint32_t kClipBlock = 256;

__device__ __forceinline__ uint32_t uniform(uint32_t v) { return __builtin_amdgcn_readfirstlane(v); }
// The tables' addresses come out of the clip's record in memory, which tells the compiler nothing of where they point: named as device
// memory here, in the pointers' types, so that the tables' accesses are global_load / global_store and not FLAT.
template <class T>
using Memory = __attribute__((address_space(1))) T*;
typedef float Row __attribute__((ext_vector_type(4)));   // (a float4 of that address space: the class type has no such assignment)
template <class T>
__device__ __forceinline__ Memory<T> in_memory(T* p) { return (Memory<T>)p; }
__device__ __forceinline__ Memory<Row> in_memory(float4* p) { return (Memory<Row>)p; }
__device__ __forceinline__ Memory<const Row> in_memory(const float4* p) { return (Memory<const Row>)p; }

__device__ __forceinline__ float4 load_row(Memory<const Row> rows, size_t i) {
  const Row v = rows[i];
  return make_float4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ void store_row(Memory<Row> rows, size_t i, float4 v) {
  Row r;
  r.x = v.x, r.y = v.y, r.z = v.z, r.w = v.w;
  rows[i] = r;
}
__device__ __forceinline__ post::Affine load_affine(Memory<const Row> rows, uint32_t b) {
  post::Affine a;
  a.r[0] = load_row(rows, 3 * (size_t)b);
  a.r[1] = load_row(rows, 3 * (size_t)b + 1);
  a.r[2] = load_row(rows, 3 * (size_t)b + 2);
  return a;
}
__device__ __forceinline__ void store_affine(Memory<Row> rows, uint32_t b, const post::Affine& a) {
  store_row(rows, 3 * (size_t)b, a.r[0]);
  store_row(rows, 3 * (size_t)b + 1, a.r[1]);
  store_row(rows, 3 * (size_t)b + 2, a.r[2]);
}

__global__ void __launch_bounds__(kClipBlock) k_clip_bones(const ClipPlay* __restrict__ plays) {
  const ClipPlay play = plays[blockIdx.x];
  const ClipArgs c = *play.clip;
  const uint32_t n_bones = uniform(c.n_bones), n_levels = uniform(c.n_levels), n_targets = uniform(c.n_targets);
  const uint32_t k0 = uniform(play.k0), k1 = uniform(play.k1);
  const float u = __uint_as_float(uniform(__float_as_uint(play.u)));
  const bool scaled = c.scales != nullptr, dq = uniform((uint32_t)play.blend) == (uint32_t)GLZ_SKIN_DUAL_QUATERNION;
  const Memory<Row> world = in_memory(c.world), bones = in_memory(c.bones);
  const Memory<const Row> inverse_bind = in_memory(c.inverse_bind);
  const Memory<const uint32_t> level_offsets = in_memory(c.level_offsets), level_bones = in_memory(c.level_bones);
  const Memory<const int32_t> parents = in_memory(c.parents);

  for (uint32_t b = threadIdx.x; b < n_bones; b += kClipBlock) store_affine(world, b, post::clip_local(in_memory(c.translations), in_memory(c.rotations), in_memory(c.scales), scaled, n_bones, b, k0, k1, u));
  __syncthreads();

  const post::Affine root = load_affine(inverse_bind, n_bones);
  uint32_t begin = uniform(level_offsets[0]);
  for (uint32_t l = 0; l < n_levels; ++l) {
    const uint32_t end = uniform(level_offsets[l + 1]);
    for (uint32_t i = begin + threadIdx.x; i < end; i += kClipBlock) {
      const uint32_t b = level_bones[i];
      const int32_t parent = parents[b];
      const post::Affine A = parent < 0 ? root : load_affine((Memory<const Row>)world, (uint32_t)parent);
      store_affine(world, b, post::affine_product(A, load_affine((Memory<const Row>)world, b)));
    }
    __syncthreads();
    begin = end;
  }

  for (uint32_t b = threadIdx.x; b < n_bones; b += kClipBlock) {
    const post::Affine B = post::affine_product(load_affine((Memory<const Row>)world, b), load_affine(inverse_bind, b));
    if (dq) {
      float4 rows[post::kSkinDqBoneRows];
      post::bone_dual_quat(B.r, rows);
      store_row(bones, post::kSkinDqBoneRows * (size_t)b, rows[0]);
      store_row(bones, post::kSkinDqBoneRows * (size_t)b + 1, rows[1]);
    } else {
      store_affine(bones, b, B);
    }
  }
  if (c.morph_weights != nullptr) {
    const Memory<const float> track = in_memory(c.morph_weights);
    const Memory<float> weights = in_memory(c.weights);
    for (uint32_t t = threadIdx.x; t < n_targets; t += kClipBlock) weights[t] = post::clip_lerp(track[(size_t)k0 * n_targets + t], track[(size_t)k1 * n_targets + t], u);
  }
}

hipError_t launch_clip_bones(hipStream_t st, const ClipPlay* plays, uint32_t n_plays) {
  if (n_plays == 0) return hipSuccess;
  hipLaunchKernelGGL(k_clip_bones, dim3(n_plays), dim3(kClipBlock), 0, st, plays);
  return hipGetLastError();
}

}  // namespace glz
