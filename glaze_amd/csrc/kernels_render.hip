// Wavefront path-tracing kernels for gfx950 (wave64).  One reference "launch" (one
// vkCmdTraceRaysKHR of path_trace.rgen = one path segment per pixel, raytracer.rs:553-562) is
// two kernels over the SoA path state in HBM:
//
//   k_trace   (persistent) ray generation / resume + closest-hit BVH4 traversal -> hit record; then the any-hit
//             traversal of the shadow rays the previous launch queued + the accumulator update (accumulate_retired)
//   k_shade   hit attributes, light sample, BSDF eval, Russian roulette, BSDF sample, state update
//             -> next ray + queued shadow ray with its contribution
//   k_finalize makes the result image and the launch count of the accumulator, once, when somebody reads the images
//
// A wave owns one 8x8 pixel block of a 64x64 tile, so primary rays of a wave are coherent and all
// per-pixel arrays are read and written as one contiguous 1 KiB (float4) line per wave.
#include "device/path_state.h"
#include "device/shade_pixel.h"
#include "device/trace_wave.h"
#include "device/trace_wave_tl.h"
#include "launch_geometry.h"
#include "symbol_readers.h"

namespace glz {
using namespace dev;

// ---------------------------------------------------------------------------------------------
// k_shade: path_trace.rgen:170-237 minus the two traceRayEXT calls, raytrace_hit.rchit:30-71
// ---------------------------------------------------------------------------------------------
// the sky's marginal cdf (H + 1 floats) is staged in LDS when it fits (the values and row integrals next to it are read once per sample, from memory: staging all 3 H + 1 floats was 12 of the 19 KB a block copies before it starts)
// (kSkyLdsFloats, device/types.h: skies of up to 1 087 rows; a taller one is searched in memory)

// (GLZ_SHADE_WAVES = 4, device/tuning.h: 128 VGPRs, 4 of them spilled, since the light's spectrum is made after the BSDF evaluation and the
// importance is read where it is used (natural demand 152 -> 132): 0.357 -> 0.348 ms; at three waves the same code takes 0.363 ms.)
// COUNT: the instrumented build of the counting passes (texture fetches, light samples: DeviceScene::tex_counter).  The measured kernel
// sets the counter pointer to a constant null, so the checks in the texture and light code fold away (left as a run-time null they
// cost 2.5 %: a branch per fetch and two more live SGPRs).
// LOD: the build with the texture level of detail (shade_pixel<LOD>).
constexpr uint32_t kShadeBlock = 256, kShadeWavesPerBlock = kShadeBlock / 64;   // the regrouping domain: pixels sorted by code path per block (512 -> 0.354 against 0.352 ms, 1 024 -> 0.368: purer waves do not pay, the kernel waits for memory)
#ifdef GLZ_SECTION_TIMES
static __device__ unsigned long long g_shade_sections[16 * 4096];   // per wave (the first 4 096 of the grid): clocks {prologue, key, sort, [shade_pixel's six], epilogue}, [15] = launches
#endif
// TABLES, SKY: whether the scene tables / the sky's marginal cdf fit their LDS areas (shade_tables_fit, shade_sky_fits: the same over the
// whole grid, so launch_shade picks the instantiation).  The address space of every table pointer is then fixed when the kernel is
// compiled -- LDS copies are read with ds_read, tables left in memory with global_load.  Chosen at run time the pointers were generic and
// every lookup a FLAT access, which goes down the vector-memory path as well and waits on both counters: what the copies are there to avoid.
__host__ __device__ inline bool shade_tables_fit(const DeviceScene& s) { return SceneTables(s).bytes() <= kShadeLdsTableBytes; }
__host__ __device__ inline bool shade_sky_fits(const DeviceScene& s) { return s.sky_header.marginal_cdf_count > 1u && s.sky_header.marginal_cdf_count <= kSkyLdsFloats; }
// a pointer into device memory, said to be one: loads through it (and through what is derived from it) are global_load
template <class T>
__device__ __forceinline__ const T* in_memory(const T* p) { return (const T*)(const __attribute__((address_space(1))) T*)p; }
template <bool COUNT, bool LOD, bool TABLES, bool SKY>
__global__ void __launch_bounds__(kShadeBlock, GLZ_SHADE_WAVES) k_shade(const LaunchArgs A) {
#ifdef GLZ_SECTION_TIMES
  unsigned long long ks[4] = {0, 0, 0, 0}, ks_last = __builtin_amdgcn_s_memtime();
#define GLZ_KS(k) do { const unsigned long long now_ = __builtin_amdgcn_s_memtime(); ks[k] += now_ - ks_last; ks_last = now_; } while (0)
#else
#define GLZ_KS(k) do { } while (0)
#endif
  // The kernel is bound by the memory system's random-access rate (16 extra scattered loads per pixel cost +27 %, 200 extra
  // VALU instructions nothing; 1 / 2 / 3 / 4 waves per SIMD take 0.76 / 0.45 / 0.36 / 0.35 ms), so the two small tables every texture fetch /
  // sky sample walks are staged in LDS once per block: the sRGB decode LUT (12 lookups per bilinear fetch) and the sky marginal CDF (an 11-step dependent search).
  __shared__ alignas(16) float s_lut[256];
  // One pool: [the importance the block's 256 pixels arrived with, 4 x 4 KB, read in whole lines by the prologue | the sky's marginal cdf |
  // the scene tables] while the block shades; after its last barrier the first 24 KB are the staging area of the state the pixels leave
  // (StagedState): 6 x 16 bytes per pixel, written where the pixel lives instead of where its thread sat.
  // (the cdf's bracket table right behind it, 33 pieces: the row search starts inside the bracket of its xi, sample_cdf)
  __shared__ uint4 s_pool[kShadeBlock * 4 + kSkyLdsFloats / 4 + kSkyBracketFloats / 4 + kShadeLdsTableBytes / 16];
  uint4* s_imp = s_pool;
  float* s_sky = reinterpret_cast<float*>(s_pool + kShadeBlock * 4);
  uint4* s_bracket = s_pool + kShadeBlock * 4 + kSkyLdsFloats / 4;
  uint4* s_tables = s_bracket + kSkyBracketFloats / 4;
  static_assert(6u * kShadeBlock <= kShadeBlock * 4 + kSkyLdsFloats / 4 + kSkyBracketFloats / 4 + kShadeLdsTableBytes / 16, "the staging area of the path state fits the pool");
  static_assert(kSkyBracketFloats / 4 <= kShadeBlock, "the bracket table is copied one piece per thread");
  // The small scene tables every hit walks through one after the other -- shading record -> RTMaterial -> texture descriptor
  // -> texels, light pick -> RTLight -- are staged in LDS when they fit: each lookup that stays on chip takes a dependent
  // memory round trip (1-2 us under load, the kernel's bound) off the hit's critical path.
  __shared__ uint32_t s_bin[kShadeWavesPerBlock * 64];   // [wave][key] counts, then start offsets
  __shared__ uint16_t s_perm[kShadeBlock];
  __shared__ float4 s_hit[kShadeBlock];   // hit records read by the regrouping prologue, handed to the thread that shades the pixel
  __shared__ float s_bounce[kShadeBlock];   // ray_o.w, the same way: all k_shade reads of ray_o unless a path restarts without pregen (StagedState::reset_origin)
  __shared__ uint2 s_pick[kShadeBlock];     // what the prologue computed for the sort key and shade_pixel needs again: {RNG state, light index} (StagedState::lds_pick)
  static_assert(kShadeBlock == 256, "pixel_of_block");
  const uint32_t n_sky = A.scene.sky_header.marginal_cdf_count;
  // both copies in 16-byte pieces, as the tables: the block pays per request, and these are a quarter of the 4-byte ones (the LUT is one
  // wave's load instead of four waves', a sky of 1 024 rows two loads per thread instead of five).  The cdf's last piece reads up to three
  // floats past it -- marginal values, which follow it in the same array (3 H + 1 floats; the pieces cover at most H + 4 of them, and exactly 4 when H = 1).
  if (threadIdx.x < 64u) reinterpret_cast<float4*>(s_lut)[threadIdx.x] = reinterpret_cast<const float4*>(A.scene.srgb_lut)[threadIdx.x];
  if (SKY) {
    for (uint32_t i = threadIdx.x; i < (n_sky + 3u) / 4u; i += kShadeBlock) s_pool[kShadeBlock * 4 + i] = reinterpret_cast<const uint4*>(A.scene.sky_marginal)[i];
    if (threadIdx.x < kSkyBracketFloats / 4) s_bracket[threadIdx.x] = reinterpret_cast<const uint4*>(A.scene.sky_marginal)[sky_bracket_offset(n_sky) / 4u + threadIdx.x];
  }
  s_bin[threadIdx.x] = 0;
  const SceneTables tables(A.scene);
  if (TABLES) tables.stage(A.scene, s_tables, kShadeBlock);
  __syncthreads();
  GLZ_KS(0);   // tables staged
  DeviceScene S = A.scene;
  unsigned long long tex_tally[4] = {0ull, 0ull, 0ull, 0ull};
  S.tex_counter = COUNT ? tex_tally : nullptr;
  S.srgb_lut = s_lut;
  S.sky_cdf = SKY ? s_sky : in_memory(S.sky_cdf);
  S.sky_rows = in_memory(S.sky_rows);
  if (TABLES) {
    tables.use(S, s_tables);
  } else {
    S.mat_compact = in_memory(S.mat_compact);
    S.metal_spectra = in_memory(S.metal_spectra);
    S.lights = in_memory(S.lights);
    S.tex_desc = in_memory(S.tex_desc);
  }
  const FrameData& F = A.frame;
  // Block-local regrouping: the 256 pixels of the block are bucketed by the code path they are going to take -- miss,
  // or (BSDF kind, light kind of the NEE sample) -- and every thread then shades the pixel at its sorted position, so
  // a wave mostly runs one material and one light routine instead of all of them one after the other (lane utilisation
  // was 32 %, SQ_THREAD_CYCLES_VALU / 64 / SQ_ACTIVE_INST_VALU, profiles/r01_pmc.json).  Pixels are independent and
  // all state is addressed by pixel, so the permutation changes no result; only the order of the shadow queue differs.
  // (The hit record requested before the tables are staged and the material id before the barrier they need -- three round trips in the
  // time of one and a half on paper: k_shade 0.326 against 0.325 ms, ten more registers spilt.  Not kept.)
  uint32_t key = 63u;   // pixels outside the image sort last
  {
    const uint32_t lid0 = blockIdx.x * kShadeBlock + threadIdx.x;
    const PixelId px0 = pixel_of_block(A.map, blockIdx.x, threadIdx.x);
    if (px0.active) {
      const float4 h0 = A.st.hit[lid0];
#pragma unroll
      for (int q = 0; q < 4; ++q) s_imp[q * kShadeBlock + threadIdx.x] = *reinterpret_cast<const uint4*>(&A.st.imp[q][lid0]);   // whole lines, pixel order (a fresh path's is never read)
      s_hit[threadIdx.x] = h0;   // the thread at this pixel's sorted slot reads it back after the barriers below: one dependent global load less
      s_bounce[threadIdx.x] = A.st.ray_o[lid0].w;   // (4 of the 16 bytes, in pixel order; the sorted thread asked for all 16, scattered)
      const uint32_t leaf0 = __float_as_uint(h0.w);
      key = 0u;
      if (leaf0 != 0xFFFFFFFFu) {
        const MatCompact* m0 = &S.mat_compact[S.two_level ? S.instances[A.st.hit_inst[lid0]].material_id : __float_as_uint(S.shade_tris[8u * (size_t)leaf0 + 6u].w)];
        // the draws shade_pixel_body starts with (DirectState::seed_rng / pick_light), made once: here, for the key, and handed on
        uint32_t light = 4u, rng0 = pixel_rng(F, px0), li0 = 0u;
        if (m0->is_specular == 0) {
          li0 = light_pick(F, rng0);
          if (F.lights_no != 0u) light = S.lights[li0].shader;
        }
        s_pick[threadIdx.x] = make_uint2(rng0, li0);
        key = 1u + (m0->bsdf_index < 6u ? m0->bsdf_index : 5u) * 5u + (light < 4u ? light : 4u);
      }
    }
  }
  GLZ_KS(1);   // hit record -> material -> code-path key
  // Counting sort without same-address atomics (256 atomicAdds on a handful of LDS words serialise: SQ_LDS_BANK_CONFLICT was
  // twice the LDS-active cycles of this kernel): every wave peels off its distinct keys with ballots -- a thread's rank among
  // the wave's threads with the same key is a popcount -- and leaves one count per (wave, key); 64 threads then turn the
  // counts into start offsets, key-major, wave-minor.
  uint32_t rank = 0;
  {
    const uint32_t wv = threadIdx.x >> 6, ln = threadIdx.x & 63u;
    unsigned long long todo = __ballot(true);
    while (todo != 0ull) {
      const uint32_t k = (uint32_t)__shfl((int)key, __ffsll((long long)todo) - 1);
      const unsigned long long m = __ballot(key == k);
      if (key == k) {
        rank = (uint32_t)__popcll(m & ((1ull << ln) - 1ull));
        if (rank == 0u) s_bin[wv * 64u + k] = (uint32_t)__popcll(m);
      }
      todo &= ~m;
    }
  }
  __syncthreads();
  if (threadIdx.x < 64) {   // exclusive prefix sum over the 64 keys of the per-key totals, then the per-wave starts inside a key
    uint32_t c[kShadeWavesPerBlock];
    uint32_t cnt = 0;
#pragma unroll
    for (uint32_t w = 0; w < kShadeWavesPerBlock; ++w) {
      c[w] = s_bin[w * 64u + threadIdx.x];
      cnt += c[w];
    }
    uint32_t incl = cnt;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const uint32_t up = __shfl_up(incl, off);
      if ((int)threadIdx.x >= off) incl += up;
    }
    uint32_t at = incl - cnt;
#pragma unroll
    for (uint32_t w = 0; w < kShadeWavesPerBlock; ++w) {
      s_bin[w * 64u + threadIdx.x] = at;
      at += c[w];
    }
  }
  __syncthreads();
  {
    const uint32_t pos = s_bin[(threadIdx.x >> 6) * 64u + key] + rank;   // the pixel's place in the block's order by code path
    s_perm[pos] = (uint16_t)threadIdx.x;
  }
  __syncthreads();
  GLZ_KS(2);   // regrouped
  const uint32_t lid = blockIdx.x * kShadeBlock + s_perm[threadIdx.x];
  // (Handing the next k_trace the pixels in this regrouped order -- one more word per pixel -- does nothing for the traversal, 0.588 ->
  // 0.591 ms; sorted per block by the octant of the new direction, camera rays last, 0.590 -> 0.573 ms, less than the sort and the
  // indirection cost.)
  const PixelId px = pixel_of_block(A.map, blockIdx.x, s_perm[threadIdx.x]);
  StagedState staged;
  if (px.active) {
    const float4 ro = make_float4(0.0f, 0.0f, 0.0f, s_bounce[s_perm[threadIdx.x]]), rd = A.st.ray_d[lid], hr = s_hit[s_perm[threadIdx.x]];
    // (see reread_kernarg: without it the regrouping prologue's view of the arguments stays in SGPRs through the shading code)
    const LaunchArgs& A2 = *(const LaunchArgs*)reread_kernarg();
    SharedQueue queue{A2};
    staged.A = &A2;
    staged.lds_imp = (LdsNodePtr)(reinterpret_cast<u32x4*>(s_imp) + s_perm[threadIdx.x]);
    staged.lds_sky_bracket = SKY ? reinterpret_cast<const uint16_t*>(s_bracket) : nullptr;
    staged.lds_pick = (StagedState::LdsPickPtr)(reinterpret_cast<StagedState::u32x2*>(s_pick) + s_perm[threadIdx.x]);
#ifdef GLZ_SECTION_TIMES
    staged.sec_last = __builtin_amdgcn_s_memtime();
#endif
    shade_pixel<LOD>(A2, S, A2.frame, lid, px, ro, rd, hr, queue, staged);
  }
#ifdef GLZ_SECTION_TIMES
  ks_last = __builtin_amdgcn_s_memtime();
#endif
  {
    // The regrouped threads would store 16-byte pieces scattered over the block's 4 KB of each state array (six arrays); the L2 has
    // to assemble the lines.  Thread i stores pixel i's state instead: the values travel through LDS, which nobody needs any more
    // once the whole block is here (a block's LDS and wave slots are handed on when its last wave ends either way).
    __syncthreads();
    float4* stage = reinterpret_cast<float4*>(s_pool);
    const uint32_t p = s_perm[threadIdx.x];   // the pixel (index in the block) this thread shaded
    s_bin[p] = staged.mask;
    if (staged.mask & 1u) stage[p] = staged.ro;
    if (staged.mask & 2u) stage[kShadeBlock + p] = staged.rd;
    if (staged.mask & 4u) {
#pragma unroll
      for (int q = 0; q < 4; ++q) stage[(2u + q) * kShadeBlock + p] = staged.im[q];
    }
    __syncthreads();
    const LaunchArgs& A3 = *(const LaunchArgs*)reread_kernarg();
    const uint32_t m = s_bin[threadIdx.x], at = blockIdx.x * kShadeBlock + threadIdx.x;
    if (m & 1u) A3.st.ray_o[at] = stage[threadIdx.x];
    if (m & 2u) A3.st.ray_d[at] = stage[kShadeBlock + threadIdx.x];
    if (m & 4u) {
#pragma unroll
      for (int q = 0; q < 4; ++q) A3.st.imp[q][at] = stage[(2u + q) * kShadeBlock + threadIdx.x];
    }
  }
  if (COUNT) flush_tex_tallies(A.counters->shade_tex, tex_tally);   // every lane of the wave is here (the counting build returns nowhere above)
#ifdef GLZ_SECTION_TIMES
  if (!COUNT) {
    GLZ_KS(3);   // the state leaves through LDS
    unsigned long long v[10] = {ks[0], ks[1], ks[2], staged.sec[0], staged.sec[1], staged.sec[2], staged.sec[3], staged.sec[4], staged.sec[5], ks[3]};
    const uint32_t w = blockIdx.x * kShadeWavesPerBlock + (threadIdx.x >> 6);
#pragma unroll
    for (int k = 0; k < 10; ++k) {   // the wave's value of a section: the largest any of its lanes saw
      unsigned int lo = (unsigned int)v[k], hi = (unsigned int)(v[k] >> 32);
      for (int off = 32; off > 0; off >>= 1) {
        const unsigned int lo2 = __shfl_xor(lo, off), hi2 = __shfl_xor(hi, off);
        const unsigned long long a = ((unsigned long long)hi << 32) | lo, b = ((unsigned long long)hi2 << 32) | lo2;
        if (b > a) { lo = lo2; hi = hi2; }
      }
      if ((threadIdx.x & 63u) == 0u && w < 4096u) g_shade_sections[16u * w + k] += ((unsigned long long)hi << 32) | lo;   // (a wave's own words: no atomics)
    }
    if ((threadIdx.x & 63u) == 0u && w < 4096u) g_shade_sections[16u * w + 15u] += 1ull;
  }
#endif
}

// ---------------------------------------------------------------------------------------------
// k_trace: ONE persistent traversal kernel per launch.  Every wave first works through its share of the closest-hit
// rays of launch L (ray generation / resume + traversal -> hit[lid]), then through its share of the shadow rays that
// launch L-1's k_shade queued (any-hit traversal, then update_count / update_result of the owning pixel).  The shadow
// test of a launch only gates an accumulation -- the path itself continues from k_shade's output -- so deferring it
// into the next launch's traversal changes no result, takes one kernel and one dependent drain off every launch's
// critical path, and lets waves that finish their closest-hit share early start on shadow rays instead of idling
// (strong scaling: at 1/8 of a 1080p frame per GPU the launch was 0.146 + 0.073 + 0.183 ms with three kernels).
// k_shade of launch L runs after this kernel, so the accumulations of launch L-1 land before those of launch L:
// the per-pixel order of `cum += c` is the reference's.
// Two counter sets: this kernel drains set shade_set ^ 1 and clears set shade_set for the k_shade that follows.
// ---------------------------------------------------------------------------------------------
template <bool COUNT, int ALPHA>
__global__ void __launch_bounds__(kBlock, GLZ_TRACE_WAVES) k_trace(const LaunchArgs A) {
  __shared__ int s_stack[kLdsStack * kBlock];
  __shared__ alignas(1024) int s_aux[kAuxPerBlock];
  __shared__ uint4 s_top[kBvhTopNodes * 4];
  static_assert(kBvhTopNodes * 4 <= kBlock, "stage_top copies one 16-byte piece per thread");
  GLZ_WAVE_STAMP(0);
  stage_top(A.scene, s_top);
  int* aux = wave_aux(s_aux, threadIdx.x >> 6);
  int* links = wave_links(s_aux, threadIdx.x >> 6);
  clear_next_queue_set(A);
  clear_next_pool_head(A);
  // counting build: the alpha tests' texture fetches are tallied through a copy of the scene that points at this thread's registers
  unsigned long long tex_tally[4] = {0ull, 0ull, 0ull, 0ull};
  DeviceScene counted_scene;
  if (COUNT) {
    counted_scene = A.scene;
    counted_scene.tex_counter = tex_tally;
  }
  const DeviceScene& TS = COUNT ? counted_scene : A.scene;
  // Waves that specialise: with more 64-ray groups than waves, a share of the waves, spread evenly over the grid wave by wave, takes only
  // shadow groups and the others only closest-hit groups: a CU holds waves of both kinds at all times.  With fewer groups than waves every
  // group gets a wave of its own either way.  The counting kernels keep the two passes per wave.
  // The division is device/trace_split.h's (one definition for host and device): the shadow waves' number, which waves they are, the shadow
  // rays [0, n_static) that are dealt to them, and the POOL [n_static, n_sh): chunks of whole groups that a wave of EITHER kind draws, one
  // returning atomic add per chunk, once its fixed share is done -- whichever kind of wave finishes first takes what is left, so neither
  // kind's fixed share has to be guessed right for every scene.  A wave that draws drains a second time, when it would otherwise be idle.
  // (Measured, that drain costs more than the idle time it fills: the default pool share is 0, everything is dealt -- device/tuning.h.)
  // Everything that steers the loops below is wave-uniform and said to be so (v_readfirstlane; see trace_wave on why the compiler must know).
  const auto uniform = [](uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); };
  const uint32_t* counts = A.st.queue_count + (A.shade_set ^ 1u) * kQueueSetWords;
  const uint32_t closest_groups = A.do_closest ? (A.map.n_local_pixels + 63u) / 64u : 0u;
  uint32_t split_closest = A.do_closest, split_wave_c = wave_index(), split_waves_c = wave_count();
  // the shadow side's first trip: when the waves do not specialise, the shadow groups are dealt out starting at the wave after the one that
  // received the last closest-hit group: with fewer groups than waves (a small tile share per GPU) every group of either kind gets a
  // wave of its own, with more the per-wave totals stay level
  uint32_t sh_trip = A.do_shadow, sh_total = 0xFFFFFFFFu /* all of them: set below */, sh_waves = wave_count(), sh_wave = (wave_index() + sh_waves - closest_groups % sh_waves) % sh_waves, sh_base = 0u;
  TraceSplit plan{0u, 0u, 0u, 0u, 0u};
  if (!COUNT && A.do_closest && A.do_shadow) {
    uint32_t n_sh = 0;
#pragma unroll
    for (uint32_t k = 0; k < kQueueShards; ++k) n_sh += counts[k * kCounterStride];
    plan = trace_split_plan(closest_groups, uniform(n_sh), wave_count(), A.split);
    if (plan.split) {
      const TraceWaveRole role = trace_split_role(plan, wave_index(), wave_count());   // the same in all lanes of a wave
      split_closest = role.is_shadow ? 0u : 1u;
      split_wave_c = role.index;    // this wave's number among the closest-hit waves (unused by a shadow wave)
      split_waves_c = wave_count() - plan.ws;
      sh_trip = role.is_shadow;     // the static sequence: shadow waves only
      sh_total = plan.n_static;
      sh_wave = role.index;         // ... or among the shadow waves
      sh_waves = plan.ws;
    }
  }
  // what of the plan the shadow side needs behind the closest-hit pass: the pool's first ray, the chunk size, the number of chunks
  const TraceSplit pool{plan.split, 0u, uniform(plan.n_static), uniform(plan.chunk_groups), uniform(plan.n_chunks)};
  split_closest = uniform(split_closest);
  if (split_closest) {
    TraceTally tally;
    ClosestSource src{A, A.frame, tally, 0u};
    ClosestSink sink{A};
    trace_wave<false, COUNT, false, GLZ_TRACE_PREFETCH != 0, false, ALPHA>(TS, src, sink, &s_stack[threadIdx.x], aux, links, (LdsNodePtr)s_top, A.st.overflow, A.st.overflow_depth, A.map.n_local_pixels, uniform(split_wave_c),
                                                         uniform(split_waves_c), tally);
    if (COUNT) flush_counters(A.counters, false, tally);
  }
  GLZ_WAVE_STAMP(1);
  if (A.do_shadow) {
    // prefix sums of the eight shard counts (final: the k_shade that filled them has completed)
    uint32_t start[kQueueShards + 1];
    start[0] = 0;
#pragma unroll
    for (uint32_t k = 0; k < kQueueShards; ++k) start[k + 1] = uniform(start[k] + counts[k * kCounterStride]);
    const uint32_t n_sh = start[kQueueShards];
    if (!pool.split) sh_total = n_sh;
    TraceTally tally;
    ShadowSource src{A, start, queue_capacity(A.map.n_local_pixels), 0u, make_float4(0.0f, 0.0f, 0.0f, 0.0f)};
    ShadowSink sink{A, src};
    // ONE trace_wave in the kernel's code: the first trip is the static sequence, every later trip a chunk drawn from the pool.  Bounded: the
    // head only grows, so a wave draws at most n_chunks + 1 times, and nothing waits for another wave.
    sh_trip = uniform(sh_trip); sh_total = uniform(sh_total); sh_wave = uniform(sh_wave); sh_waves = uniform(sh_waves);
    for (;;) {
      if (!sh_trip) {
        if (pool.n_chunks == 0u) break;
        uint32_t c = 0u;
        if ((threadIdx.x & 63u) == 0u) c = atomicAdd(A.st.queue_count + pool_head_word(A.shade_set ^ 1u), 1u);
        c = uniform(c);   // lane 0's
        if (c >= pool.n_chunks) break;
        sh_base = uniform(trace_split_chunk_first(pool, c));
        sh_total = uniform(trace_split_chunk_rays(pool, c, n_sh));   // the last chunk is short
        sh_wave = 0u;
        sh_waves = 1u;
      }
      sh_trip = 0u;
      src.base = sh_base;
      trace_wave<true, COUNT, false, GLZ_TRACE_PREFETCH != 0, false, ALPHA>(TS, src, sink, &s_stack[threadIdx.x], aux, links, (LdsNodePtr)s_top, A.st.overflow, A.st.overflow_depth, sh_total, sh_wave, sh_waves, tally);
    }
    if (COUNT) flush_counters(A.counters, true, tally);
  }
  if (COUNT) flush_tex_tallies(A.counters->trace_tex, tex_tally);
  GLZ_WAVE_STAMP(2);
}

// k_trace for a small tile share: the same two phases over the hierarchy's 8-wide nodes (trace_wave<WIDE8>).  Compiled
// for GLZ_TRACE8_WAVES waves per SIMD: a share of <= 262 144 pixels has a resident wave for every 64-ray group at four, and the node's 32
// words, the eight keys and (PREFETCH) the next node's 32 words want the registers.  No staged top, a deeper LDS stack.
__global__ void __launch_bounds__(kBlock, GLZ_TRACE8_WAVES) k_trace8(const LaunchArgs A) {
  __shared__ int s_stack[kLdsStack8 * kBlock];
  __shared__ alignas(1024) int s_aux[kAuxPerBlock];
  int* aux = wave_aux(s_aux, threadIdx.x >> 6);
  int* links = wave_links(s_aux, threadIdx.x >> 6);
  clear_next_queue_set(A);
  if (A.do_closest) {
    TraceTally tally;
    ClosestSource src{A, A.frame, tally, 0u};
    ClosestSink sink{A};
    trace_wave<false, false, false, GLZ_TRACE8_PREFETCH != 0, true>(A.scene, src, sink, &s_stack[threadIdx.x], aux, links, (LdsNodePtr) nullptr, A.st.overflow, A.st.overflow_depth,
                                                                    A.map.n_local_pixels, wave_index(), wave_count(), tally);
  }
  if (A.do_shadow) {
    const uint32_t* counts = A.st.queue_count + (A.shade_set ^ 1u) * kQueueSetWords;
    uint32_t start[kQueueShards + 1];
    start[0] = 0;
#pragma unroll
    for (uint32_t k = 0; k < kQueueShards; ++k) start[k + 1] = start[k] + counts[k * kCounterStride];
    TraceTally tally;
    ShadowSource src{A, start, queue_capacity(A.map.n_local_pixels), 0u, make_float4(0.0f, 0.0f, 0.0f, 0.0f)};
    ShadowSink sink{A, src};
    const uint32_t n_waves = wave_count();
    const uint32_t closest_groups = A.do_closest ? (A.map.n_local_pixels + 63u) / 64u : 0u;
    const uint32_t wave = (wave_index() + n_waves - closest_groups % n_waves) % n_waves;
    trace_wave<true, false, false, GLZ_TRACE8_PREFETCH != 0, true>(A.scene, src, sink, &s_stack[threadIdx.x], aux, links, (LdsNodePtr) nullptr, A.st.overflow, A.st.overflow_depth,
                                                                   start[kQueueShards], wave, n_waves, tally);
  }
}

// the same kernel for two-level scenes (trace_wave_tl): closest hits additionally record the instance
struct ClosestSinkTl {
  const LaunchArgs& A;
  __device__ __forceinline__ void store(uint32_t lid, const HitRecord& h) {
    A.st.hit[lid] = pack_hit(h);
    A.st.hit_inst[lid] = h.inst;
  }
};
// GLZ_TRACE_TL_WAVES = 4 (device/tuning.h): the instance entry and the on-the-fly world triangle need 153 VGPRs: at 6 waves per SIMD 201 of them live in scratch (forest x2000, tools/gpu_two_level_timing.py: 4.06 ms per launch), at 4 waves 34 (1.44 ms), at 3 none (1.45 ms)
template <bool COUNT>
__global__ void __launch_bounds__(kBlock, GLZ_TRACE_TL_WAVES) k_trace_tl(const LaunchArgs A) {
  __shared__ int s_stack[kLdsStack * kBlock];
  __shared__ alignas(1024) int s_aux[kAuxPerBlock];
  __shared__ float s_top_ray[9 * kBlock];   // per lane: the top level's grid-space ray (trace_wave_tl)
  __shared__ uint4 s_top[kTlLdsTop ? kBvhTopNodes * 4 : 1];
  if (kTlLdsTop) stage_top(A.scene, s_top);
  int* aux = wave_aux(s_aux, threadIdx.x >> 6);
  int* links = wave_links(s_aux, threadIdx.x >> 6);
  clear_next_queue_set(A);
  if (A.do_closest) {
    TraceTally tally;
    ClosestSource src{A, A.frame, tally, 0u};
    ClosestSinkTl sink{A};
    trace_wave_tl<false, COUNT>(A.scene, src, sink, &s_stack[threadIdx.x], aux, links, &s_top_ray[threadIdx.x], (LdsNodePtr)s_top, A.st.overflow, A.st.overflow_depth, A.map.n_local_pixels, wave_index(), wave_count(), tally);
    if (COUNT) flush_counters(A.counters, false, tally);
  }
  if (A.do_shadow) {
    const uint32_t* counts = A.st.queue_count + (A.shade_set ^ 1u) * kQueueSetWords;
    uint32_t start[kQueueShards + 1];
    start[0] = 0;
#pragma unroll
    for (uint32_t k = 0; k < kQueueShards; ++k) start[k + 1] = start[k] + counts[k * kCounterStride];
    ShadowSource src{A, start, queue_capacity(A.map.n_local_pixels), 0u, make_float4(0.0f, 0.0f, 0.0f, 0.0f)};
    ShadowSink sink{A, src};
    const uint32_t n_waves = wave_count();
    const uint32_t closest_groups = A.do_closest ? (A.map.n_local_pixels + 63u) / 64u : 0u;
    const uint32_t wave = (wave_index() + n_waves - closest_groups % n_waves) % n_waves;
    TraceTally tally;
    trace_wave_tl<true, COUNT>(A.scene, src, sink, &s_stack[threadIdx.x], aux, links, &s_top_ray[threadIdx.x], (LdsNodePtr)s_top, A.st.overflow, A.st.overflow_depth, start[kQueueShards], wave, n_waves, tally);
    if (COUNT) flush_counters(A.counters, true, tally);
  }
}

// ---------------------------------------------------------------------------------------------
// image plumbing
// ---------------------------------------------------------------------------------------------
// The resolve of a chain's images, in place (Renderer::settle; accumulate_retired / accumulate_shaded, device/path_state.h): a pixel that updated since the last
// resolve carries -(the launch of its last update) in cumulative.w, and its result is update_result's own expression with that divisor;
// the count of every active pixel is `launches`.  A pixel that never updated keeps result 0, a pixel outside the image is left alone.
__global__ void __launch_bounds__(kBlock) k_finalize(const TileMap map, float4* __restrict__ cumulative, float4* __restrict__ result, float exposure, float launches) {
  const uint32_t lid = blockIdx.x * kBlock + threadIdx.x;
  if (!pixel_of(map, lid).active) return;
  const float4 cum = cumulative[lid];
  if (cum.w < 0.0f) {
    const float w = -cum.w;
    result[lid] = make_float4(cum.x * exposure / w, cum.y * exposure / w, cum.z * exposure / w, 1.0f);
  }
  if (cum.w != launches) cumulative[lid].w = launches;
}

__global__ void __launch_bounds__(kBlock) k_export(const TileMap map, const float4* __restrict__ tiled, float4* __restrict__ frame) {
  const uint32_t lid = blockIdx.x * kBlock + threadIdx.x;
  const PixelId px = pixel_of(map, lid);
  if (px.active) frame[(size_t)px.y * map.width + px.x] = tiled[lid];
}

// chain s of S holds the rank's local tiles j = jl * S + s at chain-local index jl: lay them out in the rank's own tile order
// (what a rank of a one-process-per-GPU job sends to rank 0, 1 / world of the frame's bytes)
__global__ void __launch_bounds__(kBlock) k_pack_tiles(uint32_t n_pixels, uint32_t S, uint32_t s, const float4* __restrict__ chain, float4* __restrict__ packed) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n_pixels) return;
  const uint32_t jl = i >> 12, k = i & 4095u;
  packed[(size_t)(jl * S + s) * 4096u + k] = chain[i];
}

// linear -> sRGB OETF, 8 bit, round to nearest (what the R8G8B8A8_SRGB blit does, raytracer.rs:576-584 [ext]).
// Byte work has to be bit-exact, and pow() is not the same function on any two machines, so the quantiser is stated
// without it: q = #{k in 1..255 : c >= T_k} with T_k = (float) EOTF((k - 0.5) / 255), the smallest float whose encoded
// value rounds to k (the OETF is monotonic, so this IS round(255 * OETF(c)) evaluated exactly).  The 255 thresholds are
// computed once on the host in double precision (Renderer::allocate) and searched here from LDS: 8 compares per channel.
__device__ __forceinline__ unsigned char srgb8(const float* __restrict__ thr, float c) {
  if (!(c > 0.0f)) return 0;   // NaN, zero and negatives
  uint32_t lo = 0, hi = 255;   // invariant: c >= T_lo (T_0 = 0), c < T_(hi+1) (T_256 = +inf)
#pragma unroll
  for (int it = 0; it < 8; ++it) {
    const uint32_t mid = (lo + hi + 1u) >> 1;
    const bool ge = c >= thr[mid];
    lo = ge ? mid : lo;
    hi = ge ? hi : mid - 1u;
  }
  return (unsigned char)lo;
}
__global__ void __launch_bounds__(kBlock) k_tonemap(uint32_t n, const float4* __restrict__ result, const float* __restrict__ thresholds, uchar4* __restrict__ out) {
  __shared__ float s_thr[256];
  s_thr[threadIdx.x] = thresholds[threadIdx.x];
  __syncthreads();
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const float4 r = result[i];
  out[i] = make_uchar4(srgb8(s_thr, r.x), srgb8(s_thr, r.y), srgb8(s_thr, r.z), r.w >= 1.0f ? 255 : 0);
}


// ---------------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------------
// Blocks of k_trace's persistent grid for a chain of n_local_pixels (the renderer asks once per allocation and passes the
// answer to every launch_trace; needs the device current).  Up to one closest-hit and one shadow ray per pixel: a small
// tile share still gets a wave per 64-ray group of either kind (fewer, longer-lived waves -- 2 to 4 groups per wave --
// measured 25-50 % slower for small shares: spread as wide as possible).
uint32_t trace_grid_blocks(uint32_t n_local_pixels, bool counting, bool two_level, bool wide8) {
  uint32_t rays = 2u * n_local_pixels;
  if (wide8 && !counting && !two_level) return persistent_grid(k_trace8, rays).x;
  if (two_level) return counting ? persistent_grid(k_trace_tl<true>, rays).x : persistent_grid(k_trace_tl<false>, rays).x;   // compiled for fewer waves per SIMD: its own residency
  return counting ? persistent_grid(k_trace<true, kAlphaInline>, rays).x : std::min(persistent_grid(k_trace<false, kAlphaNone>, rays).x, persistent_grid(k_trace<false, kAlphaPhase>, rays).x);
}

hipError_t launch_trace(hipStream_t st, const LaunchArgs& a, uint32_t blocks, bool wide8) {
  if (a.map.n_local_pixels == 0) return hipSuccess;
  if (wide8 && (a.scene.two_level || a.counters || !a.scene.bvh_nodes8)) return hipErrorInvalidValue;   // the 8-wide walk: flattened scenes, no work counters
  if (blocks == 0 || (uint64_t)blocks * kBlock > 2ull * a.map.n_local_pixels + kBlock) return hipErrorInvalidValue;   // the spill area holds one slot per lane of this bound
  if (a.scene.two_level && a.counters) hipLaunchKernelGGL(k_trace_tl<true>, dim3(blocks), dim3(kBlock), 0, st, a);   // node visits of both levels, triangle tests inside the instances
  else if (a.scene.two_level) hipLaunchKernelGGL(k_trace_tl<false>, dim3(blocks), dim3(kBlock), 0, st, a);
  else if (a.counters) hipLaunchKernelGGL((k_trace<true, kAlphaInline>), dim3(blocks), dim3(kBlock), 0, st, a);
  else if (wide8) hipLaunchKernelGGL(k_trace8, dim3(blocks), dim3(kBlock), 0, st, a);
  else if (a.scene.has_non_opaque) hipLaunchKernelGGL((k_trace<false, kAlphaPhase>), dim3(blocks), dim3(kBlock), 0, st, a);   // candidates on non-opaque geometry wait for an alpha phase
  else hipLaunchKernelGGL((k_trace<false, kAlphaNone>), dim3(blocks), dim3(kBlock), 0, st, a);   // no opacity map in the scene: no alpha code in the kernel
  return hipGetLastError();
}
hipError_t launch_shade(hipStream_t st, const LaunchArgs& a) {
  if (a.map.n_local_pixels == 0) return hipSuccess;
  const dim3 grid((a.map.n_local_pixels + kShadeBlock - 1) / kShadeBlock), block(kShadeBlock);
  const int which = (a.counters ? 8 : 0) | (a.frame.lod_mode != 0u ? 4 : 0) | (shade_tables_fit(a.scene) ? 2 : 0) | (shade_sky_fits(a.scene) ? 1 : 0);
  switch (which) {
#define GLZ_SHADE_CASE(k) case k: hipLaunchKernelGGL((k_shade<((k) & 8) != 0, ((k) & 4) != 0, ((k) & 2) != 0, ((k) & 1) != 0>), grid, block, 0, st, a); break;
    GLZ_SHADE_CASE(0) GLZ_SHADE_CASE(1) GLZ_SHADE_CASE(2) GLZ_SHADE_CASE(3) GLZ_SHADE_CASE(4) GLZ_SHADE_CASE(5) GLZ_SHADE_CASE(6) GLZ_SHADE_CASE(7)
    GLZ_SHADE_CASE(8) GLZ_SHADE_CASE(9) GLZ_SHADE_CASE(10) GLZ_SHADE_CASE(11) GLZ_SHADE_CASE(12) GLZ_SHADE_CASE(13) GLZ_SHADE_CASE(14) GLZ_SHADE_CASE(15)
#undef GLZ_SHADE_CASE
  }
  return hipGetLastError();
}
hipError_t launch_finalize(hipStream_t st, const TileMap& map, float4* cumulative, float4* result, float exposure, float launches) {
  return launch_per_item(st, k_finalize, map.n_local_pixels, map, cumulative, result, exposure, launches);
}
hipError_t launch_export(hipStream_t st, const TileMap& map, const float4* tiled, float4* frame, bool zero_first) {
  if (zero_first) {
    hipError_t e = hipMemsetAsync(frame, 0, sizeof(float4) * (size_t)map.width * map.height, st);
    if (e != hipSuccess) return e;
  }
  return launch_per_item(st, k_export, map.n_local_pixels, map, tiled, frame);
}
hipError_t launch_pack_tiles(hipStream_t st, uint32_t n_chain_pixels, uint32_t n_chains, uint32_t chain, const float4* tiled, float4* packed) {
  return launch_per_item(st, k_pack_tiles, n_chain_pixels, n_chain_pixels, n_chains, chain, tiled, packed);
}
hipError_t launch_tonemap(hipStream_t st, uint32_t n, const float4* result_frame, const float* thresholds, uchar4* out) {
  static_assert(kBlock == 256, "k_tonemap stages the 256 thresholds with one load per thread");
  hipLaunchKernelGGL(k_tonemap, grid_for(n), dim3(kBlock), 0, st, n, result_frame, thresholds, out);
  return hipGetLastError();
}

}  // namespace glz

#ifdef GLZ_SECTION_TIMES
extern "C" int glz_debug_shade_sections(unsigned long long* out, int reset) { return glz::read_device_symbol(out, glz::g_shade_sections, sizeof(glz::g_shade_sections), reset); }
// kernels_render.hip and kernels_path.hip each hold their own copy of g_sections (a __device__ array per translation unit): `which` 0 = k_trace's, see kernels_path.hip for k_path's
extern "C" int glz_debug_sections_trace(unsigned long long* out, int reset) { return glz::read_device_symbol(out, glz::g_sections, sizeof(glz::g_sections), reset); }
#endif
#ifdef GLZ_WAVE_TIMES
extern "C" int glz_debug_wave_times(unsigned long long* out, int n_waves) {
  if (n_waves > 8192) n_waves = 8192;
  return glz::read_device_symbol(out, glz::g_wave_times, sizeof(unsigned long long) * 3 * (size_t)n_waves, 0);
}
extern "C" int glz_debug_tl_stats(unsigned long long* out, int reset) {
  int e = (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(glz::g_tl_stats), sizeof(unsigned long long) * 8);
  if (reset && e == 0) {
    const unsigned long long zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    e = (int)hipMemcpyToSymbol(HIP_SYMBOL(glz::g_tl_stats), zero, sizeof(zero));
  }
  return e;
}
extern "C" int glz_debug_wave_stats(unsigned int* out, int n_waves) {
  if (n_waves > 8192) n_waves = 8192;
  return glz::read_device_symbol(out, glz::g_wave_stats, sizeof(unsigned int) * 8 * (size_t)n_waves, 0);
}
#endif
