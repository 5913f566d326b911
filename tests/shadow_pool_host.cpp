// Host check of k_trace's division of a launch (glaze_amd/csrc/device/trace_split.h), compiled and run by tests/test_shadow_pool_host.py.
// The header is the one the kernel includes.  What it must give, for every input below:
//   * every shadow ray index in [0, n_sh) lies in exactly one place: the static sequence of exactly one shadow wave (the deal of
//     device/trace_wave.h RaySequence over [0, n_static), restated here) or exactly one pool chunk;
//   * 1 <= ws <= nw - 1, the shadow waves are numbered 0 .. ws - 1 and the closest-hit waves 0 .. nw - ws - 1, each number once;
//   * with a pool share of 0 the division is the one k_trace had before there was a pool -- that formula is restated here, not included.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "device/trace_split.h"

using glz::TraceSplit;
using glz::TraceSplitTuning;

static unsigned long long wrong = 0, cases = 0, split_cases = 0;
#define CHECK(cond, ...)                                  \
  do {                                                    \
    if (!(cond)) {                                        \
      if (wrong < 20) { printf("WRONG %s: ", #cond); printf(__VA_ARGS__); printf("\n"); } \
      ++wrong;                                            \
    }                                                     \
  } while (0)

// the division before the pool, as kernels_render.hip had it (GLZ_TRACE_SPLIT_NUM / _DEN = num / den)
struct Old {
  bool split;
  uint32_t ws;
};
static Old old_plan(uint32_t gc, uint32_t n_sh, uint32_t nw, uint32_t num, uint32_t den) {
  const uint32_t gs = (n_sh + 63u) / 64u;
  Old o{false, 0u};
  if (nw >= 2u && gc + gs > nw && gs > 0u) {   // (a grid has at least four waves; with one wave there is nothing to divide)
    o.split = true;
    uint32_t ws = (uint32_t)(((unsigned long long)nw * gs * num) / ((unsigned long long)gc * den + (unsigned long long)gs * num));
    o.ws = ws < 1u ? 1u : (ws > nw - 1u ? nw - 1u : ws);
  }
  return o;
}

static std::vector<uint8_t> seen;

static void check(uint32_t gc, uint32_t n_sh, uint32_t nw, const TraceSplitTuning& t) {
  ++cases;
  const TraceSplit p = glz::trace_split_plan(gc, n_sh, nw, t);
  const Old o = old_plan(gc, n_sh, nw, t.static_num, t.static_den);
  CHECK((p.split != 0u) == o.split, "gc %u n_sh %u nw %u", gc, n_sh, nw);
  if (!p.split) {
    CHECK(p.n_chunks == 0u && p.ws == 0u, "gc %u n_sh %u nw %u: no split, but chunks %u ws %u", gc, n_sh, nw, p.n_chunks, p.ws);
    return;
  }
  ++split_cases;
  CHECK(p.ws == o.ws, "gc %u n_sh %u nw %u: ws %u, formula %u", gc, n_sh, nw, p.ws, o.ws);
  CHECK(p.ws >= 1u && p.ws <= nw - 1u, "gc %u n_sh %u nw %u: ws %u", gc, n_sh, nw, p.ws);
  CHECK(p.n_static <= n_sh && (p.n_static % 64u == 0u || p.n_static == n_sh), "n_sh %u: n_static %u", n_sh, p.n_static);
  CHECK(p.chunk_groups >= 1u, "chunk %u", p.chunk_groups);
  if (t.pool_num == 0u) CHECK(p.n_static == n_sh && p.n_chunks == 0u, "pool off: n_sh %u n_static %u chunks %u", n_sh, p.n_static, p.n_chunks);
  if (t.pool_num == t.pool_den) CHECK(p.n_static == 0u, "pool share 1: n_static %u", p.n_static);
  // the waves' roles
  uint32_t n_shadow = 0, n_closest = 0;
  seen.assign(n_sh, 0);
  for (uint32_t w = 0; w < nw; ++w) {
    const glz::TraceWaveRole r = glz::trace_split_role(p, w, nw);
    const uint32_t s_before = (uint32_t)(((unsigned long long)w * o.ws) / nw), s_after = (uint32_t)(((unsigned long long)(w + 1u) * o.ws) / nw);
    CHECK((r.is_shadow != 0u) == (s_after > s_before), "wave %u of %u, ws %u", w, nw, o.ws);
    if (r.is_shadow) {
      CHECK(r.index == n_shadow && r.count == p.ws, "shadow wave %u: index %u of %u, expected %u of %u", w, r.index, r.count, n_shadow, p.ws);
      ++n_shadow;
      // its static sequence: RaySequence(r.index, r.count, n_static), ray_at(pos) = (wave + (pos >> 6) * n_waves) * 64 + (pos & 63) while < total
      for (uint32_t pos = 0;; ++pos) {
        const unsigned long long ray = ((unsigned long long)r.index + (unsigned long long)(pos >> 6) * r.count) * 64u + (pos & 63u);
        if (ray >= p.n_static) {
          if ((pos & 63u) == 0u) break;   // the sequence has ended (ray_at is monotonic from a group's first ray on)
          pos |= 63u;                     // a short last group: on to the next group's first ray, which ends it
          continue;
        }
        seen[ray] += 1;
      }
    } else {
      CHECK(r.index == n_closest && r.count == nw - p.ws, "closest wave %u: index %u of %u, expected %u of %u", w, r.index, r.count, n_closest, nw - p.ws);
      ++n_closest;
    }
  }
  CHECK(n_shadow == p.ws && n_closest == nw - p.ws, "ws %u: %u shadow + %u closest waves of %u", p.ws, n_shadow, n_closest, nw);
  // the pool's chunks
  for (uint32_t c = 0; c < p.n_chunks; ++c) {
    const uint32_t first = glz::trace_split_chunk_first(p, c);
    CHECK(first < n_sh, "chunk %u of %u starts at %u of %u", c, p.n_chunks, first, n_sh);
    if (first >= n_sh) continue;
    const uint32_t rays = glz::trace_split_chunk_rays(p, c, n_sh);
    CHECK(rays >= 1u && rays <= p.chunk_groups * 64u && first + rays <= n_sh, "chunk %u: %u rays from %u of %u", c, rays, first, n_sh);
    for (uint32_t i = 0; i < rays && first + i < n_sh; ++i) seen[first + i] += 1;
  }
  uint32_t bad = 0;
  for (uint32_t i = 0; i < n_sh; ++i) bad += seen[i] != 1;
  CHECK(bad == 0u, "gc %u n_sh %u nw %u, static %u/%u pool %u/%u chunk %u: %u rays not in exactly one place (ws %u n_static %u chunks %u)", gc, n_sh, nw, t.static_num,
        t.static_den, t.pool_num, t.pool_den, t.chunk_groups, bad, p.ws, p.n_static, p.n_chunks);
}

int main() {
  const uint32_t waves[] = {1u, 2u, 7u, 1024u, 6144u};
  const uint32_t pools[][2] = {{0u, 1u}, {1u, 8u}, {1u, 4u}, {1u, 2u}, {1u, 1u}};
  const uint32_t chunks[] = {1u, 2u, 4u, 1u << 20};   // the last: larger than any pool here
  for (uint32_t nw : waves) {
    std::vector<uint32_t> gcs = {0u, 1u, nw / 2u, nw, nw + 1u, 3u * nw}, rays = {0u, 1u, 63u, 64u, 65u, 64u * nw - 1u, 64u * nw, 64u * nw + 1u, 2u * 64u * nw + 17u, 3u * 64u * nw + 64u};
    if (nw <= 7u)
      for (uint32_t n = 0; n <= 4u * 64u * nw; n += 13u) rays.push_back(n);
    for (uint32_t gc : gcs)
      for (uint32_t n_sh : rays)
        for (uint32_t num = 5u; num <= 8u; ++num)
          for (const auto& pool : pools)
            for (uint32_t chunk : chunks) check(gc, n_sh, nw, TraceSplitTuning{num, 10u, pool[0], pool[1], chunk});
  }
  printf("%llu inputs checked (%llu divide the waves), %llu wrong\n", cases, split_cases, wrong);
  return wrong ? 1 : 0;
}
