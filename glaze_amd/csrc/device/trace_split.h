// How one k_trace launch divides its 64-ray groups among its waves: ONE definition, plain integers, for the kernel (kernels_render.hip),
// the host (Renderer::fill_args fills the tuning values) and the host test (tests/shadow_pool_host.cpp).
//
// With more groups than waves the waves specialise: `ws` of the `nw` waves, spread evenly over the grid, take only shadow groups, the
// others only closest-hit groups.  The shadow rays [0, n_static) are dealt to the shadow waves round-robin, group by
// group, as before; the rest, [n_static, n_sh), is the POOL: chunks of `chunk_groups` groups that whichever wave finishes its fixed share
// first -- of either kind -- draws with one returning atomic add per chunk.  A pool share of 0 leaves today's division: everything dealt.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace glz {

// The tuning values (device/tuning.h holds the defaults and what they were measured against); they travel in LaunchArgs.
struct TraceSplitTuning {
  uint32_t static_num, static_den;   // the shadow waves' share relative to the shadow groups' share of all groups
  uint32_t pool_num, pool_den;       // the fraction of the shadow groups that is left undealt
  uint32_t chunk_groups;             // groups a wave draws from the pool at a time
};

struct TraceSplit {
  uint32_t split;          // 0: the waves do not specialise (no more groups than waves, or no shadow ray); the other fields are then 0
  uint32_t ws;             // shadow waves, 1 <= ws <= nw - 1
  uint32_t n_static;       // shadow rays [0, n_static) are dealt to the shadow waves; a whole number of groups unless it is all of n_sh
  uint32_t chunk_groups;   // >= 1
  uint32_t n_chunks;       // chunks of the pool: chunk c holds the rays [n_static + c * chunk_groups * 64, ... + chunk_groups * 64) below n_sh
};

// gc: closest-hit groups, n_sh: shadow rays, nw: waves of the grid
__host__ __device__ inline TraceSplit trace_split_plan(uint32_t gc, uint32_t n_sh, uint32_t nw, const TraceSplitTuning& t) {
  TraceSplit p{0u, 0u, 0u, 0u, 0u};
  const uint32_t gs = (n_sh + 63u) / 64u;
  if (nw < 2u || gs == 0u || (unsigned long long)gc + gs <= nw) return p;
  p.split = 1u;
  const unsigned long long s_part = (unsigned long long)gs * t.static_num, c_part = (unsigned long long)gc * t.static_den;
  const uint32_t ws = s_part + c_part ? (uint32_t)(((unsigned long long)nw * s_part) / (c_part + s_part)) : 0u;
  p.ws = ws < 1u ? 1u : (ws > nw - 1u ? nw - 1u : ws);
  uint32_t pool_groups = t.pool_den ? (uint32_t)(((unsigned long long)gs * t.pool_num) / t.pool_den) : 0u;
  pool_groups = pool_groups > gs ? gs : pool_groups;
  p.n_static = pool_groups ? (gs - pool_groups) * 64u : n_sh;   // (the queue's last, short group is the pool's when there is one)
  p.chunk_groups = t.chunk_groups < 1u ? 1u : t.chunk_groups;
  p.n_chunks = (pool_groups + p.chunk_groups - 1u) / p.chunk_groups;
  return p;
}

// first ray and number of rays of pool chunk c < n_chunks (the last chunk may be short)
__host__ __device__ inline uint32_t trace_split_chunk_first(const TraceSplit& p, uint32_t c) { return p.n_static + c * p.chunk_groups * 64u; }
__host__ __device__ inline uint32_t trace_split_chunk_rays(const TraceSplit& p, uint32_t c, uint32_t n_sh) {
  const uint32_t first = trace_split_chunk_first(p, c), left = n_sh - first;
  return left < p.chunk_groups * 64u ? left : p.chunk_groups * 64u;
}

// Which waves are shadow waves (p.split != 0): wave w is one where floor((w + 1) ws / nw) steps past floor(w ws / nw), which spreads
// them evenly over the grid; `index` is the wave's number among the `count` waves of its own kind.
struct TraceWaveRole {
  uint32_t is_shadow, index, count;
};
__host__ __device__ inline TraceWaveRole trace_split_role(const TraceSplit& p, uint32_t w, uint32_t nw) {
  const uint32_t s_before = (uint32_t)(((unsigned long long)w * p.ws) / nw), s_after = (uint32_t)(((unsigned long long)(w + 1u) * p.ws) / nw);
  TraceWaveRole r;
  r.is_shadow = s_after > s_before ? 1u : 0u;
  r.index = r.is_shadow ? s_before : w - s_before;
  r.count = r.is_shadow ? p.ws : nw - p.ws;
  return r;
}

}  // namespace glz
