// The path state as the tracers see it: pixel <-> thread mapping, the camera ray, the ray sources and sinks of the closest-hit and
// the shadow pass, the accumulator update and the shadow-ray queue.
#pragma once
#include <hip/hip_runtime.h>

#include "device/intersect.h"
#include "device/math.h"
#include "device/trace_wave.h"
#include "kernels.h"

namespace glz {
using namespace dev;

constexpr uint32_t kQueueShards = 8;     // shadow-ray sub-queues (see queue_slot)
constexpr uint32_t kCounterStride = 32;  // uint32 words between shard counters (128 bytes)
constexpr uint32_t kFlagUpdate = 1u;    // update_result() is called for this pixel in this launch
constexpr uint32_t kFlagShadow = 2u;    // the contribution is gated by a shadow ray

// ---------------------------------------------------------------------------------------------
// pixel <-> thread mapping
// ---------------------------------------------------------------------------------------------
struct PixelId {
  uint32_t x, y;
  bool active;
};
__device__ __forceinline__ PixelId pixel_of(const TileMap& m, uint32_t lid) {
  const uint32_t lane = lid & 63u, sub = (lid >> 6) & 63u, ltile = lid >> 12;
  const uint32_t gtile = ltile * m.world + m.rank;
  const uint32_t tx = gtile % m.tiles_x, ty = gtile / m.tiles_x;
  PixelId p;
  p.x = tx * 64u + (sub & 7u) * 8u + (lane & 7u);
  p.y = ty * 64u + (sub >> 3) * 8u + (lane >> 3);
  p.active = lid < m.n_local_pixels && p.x < m.width && p.y < m.height;
  return p;
}
// pixel_of(m, block * 256 + p) for p < 256: the 256 pixels share a tile, so the tile's place in the frame -- the division -- is computed
// from the block number alone, once per wave on the scalar unit, whichever pixel of the block a thread then turns to
__device__ __forceinline__ PixelId pixel_of_block(const TileMap& m, uint32_t block, uint32_t p) {
  const uint32_t gtile = (block >> 4) * m.world + m.rank;
  const uint32_t tx = gtile % m.tiles_x, ty = gtile / m.tiles_x;
  const uint32_t lane = p & 63u, sub = (block & 15u) * 4u + (p >> 6);
  PixelId px;
  px.x = tx * 64u + (sub & 7u) * 8u + (lane & 7u);
  px.y = ty * 64u + (sub >> 3) * 8u + (lane >> 3);
  px.active = block * 256u + p < m.n_local_pixels && px.x < m.width && px.y < m.height;
  return px;
}

// ---------------------------------------------------------------------------------------------
// closest-hit phase of k_trace: path_trace.rgen:143-169
// ---------------------------------------------------------------------------------------------
// (k_path with a wave's 64 pixels dealt from 4 ... 64 different groups, to average the groups' persistent cost differences: it does at a
// half-empty machine and not at a 1/8 share, where the coherence lost costs more: EXPERIMENTS.md.)
// The camera ray of a new path through the jittered pixel (ray_origin / ray_dir, path_trace.rgen:47-73).  Two callers, the same
// operations in the same order: the traversal kernel's refill for a pixel whose path is new and has no ray yet (the first launch after
// a restart, the direct-light integrator), and the shading code for a path that has just ended, with the NEXT launch's pixel offset.
__device__ __forceinline__ void camera_ray(const LaunchArgs& A, const FrameData& F, PixelId px, float off_x, float off_y, vec3& origin, vec3& direction) {
  const float pxf = (float)px.x + off_x, pyf = (float)px.y + off_y;
  const float ndcx = -1.0f + 2.0f * (pxf / F.scene_size[0]), ndcy = -1.0f + 2.0f * (pyf / F.scene_size[1]);
  const float* c2w = A.cam.camera2world;
  const float* s2c = A.cam.screen2camera;
  const float ortho = gl_step(0.5f, F.camera_persp ? 0.0f : 1.0f), persp = gl_step(0.5f, F.camera_persp ? 1.0f : 0.0f);
  const float ox = ndcx * ortho, oy = ndcy * ortho;
  origin = mk3((c2w[0] * ox + c2w[4] * oy) + c2w[12], (c2w[1] * ox + c2w[5] * oy) + c2w[13], (c2w[2] * ox + c2w[6] * oy) + c2w[14]);
  const float fx = ndcx * persp, fy = ndcy * persp;
  const vec3 target = mk3(((s2c[0] * fx + s2c[4] * fy) + s2c[8]) + s2c[12], ((s2c[1] * fx + s2c[5] * fy) + s2c[9]) + s2c[13],
                          ((s2c[2] * fx + s2c[6] * fy) + s2c[10]) + s2c[14]);
  const vec3 nt = normalize3(target);
  const float dx = (c2w[0] * nt.x + c2w[4] * nt.y) + c2w[8] * nt.z, dy = (c2w[1] * nt.x + c2w[5] * nt.y) + c2w[9] * nt.z;
  const float dz = (c2w[2] * nt.x + c2w[6] * nt.y) + c2w[10] * nt.z, dw = (c2w[3] * nt.x + c2w[7] * nt.y) + c2w[11] * nt.z;
  const float inv = 1.0f / sqrtf(((dx * dx + dy * dy) + dz * dz) + dw * dw);   // normalize() of the vec4
  direction = mk3(dx * inv, dy * inv, dz * inv);
}
// ray_o.w of a pixel is the bounce its path is at; 0 = a new path.  +0.0: the camera ray is still to be made (by the refill below);
// -0.0 (kPregenBounce): the shading code of the previous launch has made it already (shade_pixel) and ray_o / ray_d hold it.  Both
// compare equal to 0.0f, which is all the shading code asks.
constexpr uint32_t kPregenBounceBits = 0x80000000u;
struct ClosestSource {
  const LaunchArgs& A;
  const FrameData& F;   // the launch's constants (k_trace: A.frame; k_path: one entry of its batch)
  TraceTally& tally;
  uint32_t base;        // ray i is local pixel base + i (k_trace: 0; k_path: the first pixel of the wave's group)
  // ray generation / resume for local pixel `lid`
  // (Dealing the rays of a group from 4, 16 or 64 different tiles instead of one row of one tile -- to level the waves of a small
  // share, whose ends spread from 60 (median) to 105 us -- changes nothing: the spread is not regional, a wave is as slow as the
  // longest dependent chain among its 64 rays.  Median and end of the phase moved by +3 ... +8 % with the coherence lost.)
  __device__ __forceinline__ bool load(uint32_t i, vec3& origin, vec3& direction, float& tmin, float& tmax) {
    const uint32_t lid = base + i;
    if (lid >= A.map.n_local_pixels) return false;
    const float4 ro = A.st.ray_o[lid], rd = A.st.ray_d[lid];
    // A refill runs with the 16 - 24 lanes that were idle, and a quarter of the pixels start a new path in every launch: making their
    // camera rays here -- ~170 VALU instructions with four divisions and two square roots, at a quarter of the lanes, in nearly every
    // refill of a kernel that is bound by VALU issue -- was 8 % of k_trace's instructions.  The shading code makes them now where the
    // paths end (whole waves of misses after k_shade's regrouping), and the branch below is taken by the launch after a restart only.
    // (Where the pixel is -- a division by the tiles per row -- only matters here: the pixels of an edge tile that lie outside the image
    // are never written by anybody, stay at +0.0 and come this way in every launch.)
    if (F.direct_only || __float_as_uint(ro.w) == 0u) {
      const PixelId px = pixel_of(A.map, lid);
      if (!px.active) return false;
      tally.fresh += 1;
      camera_ray(A, F, px, F.pixel_offset[0], F.pixel_offset[1], origin, direction);
      A.st.ray_o[lid] = make_float4(origin.x, origin.y, origin.z, ro.w);
      A.st.ray_d[lid] = make_float4(direction.x, direction.y, direction.z, rd.w);
    } else {
      if (ro.w == 0.0f) tally.fresh += 1;
      origin = mk3(ro.x, ro.y, ro.z);
      direction = mk3(rd.x, rd.y, rd.z);
    }
    tmin = 0.0001f;
    tmax = INFINITY;
    return true;
  }
};
// the closest-hit record as it is stored: (t (inf = miss), u, v, leaf bits)
__device__ __forceinline__ float4 pack_hit(const HitRecord& h) { return make_float4(h.leaf == 0xFFFFFFFFu ? INFINITY : h.t, h.u, h.v, __uint_as_float(h.leaf)); }
struct ClosestSink {
  const LaunchArgs& A;
  __device__ __forceinline__ void store(uint32_t lid, const HitRecord& h) { A.st.hit[lid] = pack_hit(h); }
};

// update_count() + update_result() of path_trace.rgen:119-133 for one pixel, with the result left to k_finalize.  update_count runs once
// per active pixel and accumulating launch -- a miss, a specular hit, a hit without a light sample, a shadow ray retired either way -- so
// the count of every active pixel is the same number, which the host knows, and a pixel that does not update touches no memory.  What is
// per pixel is the launch of its last update_result: `mark`, -(float)min(u, 2^24) for the u-th accumulating launch since the reset, goes
// to cumulative.w.  The sign says "updated since the last resolve", the magnitude is what update_result divided by (the eager
// w += 1.0f sticks at 2^24 too); k_finalize (kernels_render.hip) makes result and the count from it whenever somebody looks.
// accumulate_retired: a shadow ray's end (k_trace, k_path).  An occluded ray has nothing to add: four bytes say that the pixel updated, the
// accumulator is not read.  `cum` = cumulative[lid] as read by the caller (only its xyz are used, and only by an unoccluded ray).
// accumulate_shaded: the shading code's update.  `add` false -- a hit without a light sample, whose contribution is exactly (+0, +0, +0),
// or a non-finite sample, which adds nothing -- marks the pixel like an occluded ray does: four bytes, the accumulator is not read.
// That leaves the bits the read-modify-write left, sum + (+0.0) == sum, unless a component of the sum is -0.0.  None ever is:
// the sums start at +0.0 (Renderer::reset_buffers fills the array with zero bytes for every new frame), a round-to-nearest sum is -0.0 only when
// both operands are, so by induction over the additions here and in accumulate_retired no sum becomes -0.0 whatever is added;
// k_finalize writes .w only, and DeviceGroup's gather / scatter paths (k_export, k_pack_tiles) read the array and never write it.
__device__ __forceinline__ float update_mark(uint32_t ordinal) { return -(float)(ordinal < (1u << 24) ? ordinal : (1u << 24)); }
__device__ __forceinline__ void accumulate_retired(const LaunchArgs& A, uint32_t lid, vec3 c, bool add, float mark, float4 cum) {
  if (add) A.st.cumulative[lid] = make_float4(cum.x + c.x, cum.y + c.y, cum.z + c.z, mark);
  else A.st.cumulative[lid].w = mark;
}
__device__ __forceinline__ void accumulate_shaded(const LaunchArgs& A, uint32_t lid, vec3 c, bool add, bool update, float mark) {
  if (!update) return;
  if (add) {
    const float4 cum = A.st.cumulative[lid];
    A.st.cumulative[lid] = make_float4(cum.x + c.x, cum.y + c.y, cum.z + c.z, mark);
  } else {
    A.st.cumulative[lid].w = mark;
  }
}

// Shadow-ray queue: 8 sub-queues ("shards"), shard = blockIdx % 8.  Blocks b and b+8 are observed to land on
// the same XCD, so a shard's counter line tends to stay in one XCD's L2; more importantly eight counters on
// separate 128-byte lines take eight times the append rate of one word (MI355X_MICROARCH.md, row `dequeue`).
// A shard only receives entries from its own blocks, so its capacity ceil(blocks/8) * kBlock can never overflow.
__device__ __forceinline__ uint32_t queue_capacity(uint32_t n_local_pixels) {
  const uint32_t blocks = (n_local_pixels + kBlock - 1) / kBlock;
  return ((blocks + kQueueShards - 1) / kQueueShards) * kBlock;
}
// Appends the lanes with `push` set: one atomic per wave (ballot + popcount); the wave's entries are contiguous so
// the three float4 stores stay coalesced.  Returns the entry index in the queue arrays.
__device__ __forceinline__ uint32_t queue_slot(uint32_t* counters, uint32_t n_local_pixels, bool push) {
  const unsigned long long m = __ballot(push);
  uint32_t slot = 0;
  if (push) {
    const uint32_t shard = ((blockIdx.x * blockDim.x + threadIdx.x) / kBlock) % kQueueShards;   // by 256-pixel segment, whatever the block size (queue_capacity)
    const int lane = threadIdx.x & 63;
    const int leader = __ffsll((long long)m) - 1;
    uint32_t base = 0;
    if (lane == leader) base = atomicAdd(counters + shard * kCounterStride, (uint32_t)__popcll(m));
    base = __shfl(base, leader);
    slot = shard * queue_capacity(n_local_pixels) + base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
  }
  return slot;
}

// ---------------------------------------------------------------------------------------------
// Shadow rays: the shadow traceRayEXT (path_trace.rgen:106-110) for the compacted queue written by k_shade,
// followed by update_count / update_result (:119-133, accumulate_retired) of the owning pixel (source / sink of k_trace's second phase).
// ---------------------------------------------------------------------------------------------
struct ShadowSource {
  const LaunchArgs& A;
  const uint32_t* start;   // prefix sums of the shard counts (kQueueShards + 1 entries)
  uint32_t cap;
  uint32_t lid;            // per-lane: owning pixel and contribution of the ray in flight
  float4 contrib;
  uint32_t base = 0u;      // wave-uniform: ray i of a call is queue ray base + i (k_trace: the first ray of a chunk drawn from the pool; 0 everywhere else)
  __device__ __forceinline__ bool load(uint32_t i, vec3& o, vec3& d, float& tmin, float& tmax) {
    i += base;
    uint32_t shard = 0;
#pragma unroll
    for (uint32_t k = 1; k < kQueueShards; ++k) shard += i >= start[k] ? 1u : 0u;
    const uint32_t q = shard * cap + (i - start[shard]);
    const float4 so = A.st.sh_o[q], sd = A.st.sh_d[q];
    contrib = A.st.contrib[q];
    lid = __float_as_uint(sd.w);
    o = mk3(so.x, so.y, so.z);
    d = mk3(sd.x, sd.y, sd.z);
    tmin = 0.001f;
    tmax = so.w;
    return true;
  }
};
struct ShadowSink {
  const LaunchArgs& A;
  ShadowSource& src;
  __device__ __forceinline__ void store(uint32_t, const HitRecord& h) {
    const bool occluded = h.leaf != 0xFFFFFFFFu;
    const vec3 c = mk3(src.contrib.x, src.contrib.y, src.contrib.z);
    if (occluded) A.st.cumulative[src.lid].w = A.shadow_mark;   // no read: the sum stays
    else accumulate_retired(A, src.lid, c, true, A.shadow_mark, A.st.cumulative[src.lid]);
  }
};
// every tracing kernel clears the counters of the queue set the k_shade that follows fills (shade_set)
__device__ __forceinline__ void clear_next_queue_set(const LaunchArgs& A) {
  if (blockIdx.x == 0 && threadIdx.x < kQueueShards) A.st.queue_count[A.shade_set * kQueueSetWords + threadIdx.x * kCounterStride] = 0;
}
// k_trace, both the product's and the counting one: with them the head of that set's shadow-group pool (kernels.h pool_head_word) -- the
// k_trace that drains the set in the next launch draws from it, this one draws from the other set's.  The other tracers need not: which
// tracer runs a chain's launches only changes with a reallocation, which restarts (Renderer::reset_buffers clears both heads), or with
// the work counters, which swap k_trace for its own counting instantiation.
__device__ __forceinline__ void clear_next_pool_head(const LaunchArgs& A) {
  if (blockIdx.x == 0 && threadIdx.x == kQueueShards) A.st.queue_count[pool_head_word(A.shade_set)] = 0;
}
}  // namespace glz
