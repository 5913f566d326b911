// The wave-persistent tracer of the flattened scene (trace_wave) and what every kernel built on a tracer declares and calls: the
// LDS stack, the block's scratch layout, the staged top of the tree, the wave's place in the grid, the counting kernels' flushes.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "device/intersect.h"
#include "device/sort4.h"
#include "device/tuning.h"
#include "device/types.h"
#include "kernels.h"

namespace glz {
using namespace dev;

constexpr int kBlock = (int)kTraceBlock;   // 4 waves
constexpr int kLdsStack = kTraversalLdsStack;   // stack entries kept in LDS per lane (17 levels: 17.4 KB of the 25.3 KB a k_trace block takes -> 6 blocks per CU); deeper levels spill to HBM

// Per-lane traversal stack: the first kLdsStack levels in LDS (column `tid` of a [level][kBlock]
// array, accessed with 4-byte DS instructions, which gfx950 services in two 32-lane halves with bank = (addr / 4) % 32
// -- the 64-bank mapping only applies to the 8- and 16-byte reads: every lane hits bank tid % 32 of its own half,
// conflict-free whatever the per-lane depth), deeper
// levels in a per-lane HBM spill area.  kStolen marks an LDS entry that was handed to an idle lane (work sharing
// at the tail of trace_wave); pop_live() skips such entries.
constexpr int kRayDone = 0x7FFFFFFF;   // `cur` of a lane without a node to visit (inner nodes are >= 0, leaves < 0)
constexpr int kStolen = 0x7FFFFFFE;
// The LDS column is addressed through a pointer that KEEPS its address space: with a generic pointer the compiler turned pop() -- LDS
// level or spilt level -- into ONE flat_load_dword behind a pointer select, i.e. every pop of the traversal went through the flat path
// and waited for vmcnt(0) AND lgkmcnt(0) (with it all of the lane's loads in flight): the largest single piece of a node iteration
// (tools/gpu_sections.py, round 4: ~1 000 of ~2 400 clocks on an otherwise idle chip).  The staged top of the tree had the same
// problem in round 2 (LdsNodePtr).
typedef __attribute__((address_space(3))) int* LdsIntPtr;
// Record `index` of a table in memory, addressed as the table's (wave-uniform) base plus a 32-bit BYTE offset per lane: the load
// is global_load_dwordx4 v, vOffset, s[base:base+1] behind one v_lshlrev_b32, where `table + index` with a signed index makes the address
// in 64 bits per lane (v_mov 0, v_lshlrev_b64, v_lshl_add_u64).  No table of the hierarchy reaches 2^32 bytes: the host refuses such a
// scene (kernels.h traversal_offsets_exceeded) -- the links alone, 30 bits of node or leaf number, would allow sixteen times that.
template <class T>
__device__ __forceinline__ const T* record_at(const T* table, uint32_t index) {
  return reinterpret_cast<const T*>(reinterpret_cast<const char*>(table) + index * (uint32_t)sizeof(T));
}
// this lane's slot of the grid's spill area (a lane traverses one ray or subtree at a time)
__device__ __forceinline__ uint32_t lane_slot() { return (blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6)) * 64u + (threadIdx.x & 63u); }
template <int kLevels>
struct StackT {
  LdsIntPtr lds;        // &s_stack[threadIdx.x]
  char* spill;          // the grid's overflow area (wave-uniform) ...
  uint32_t spill_off;   // ... and the byte offset of this lane's words in it (the whole area is shorter than 2^32 bytes: traversal_offsets_exceeded)
  int sp;
  __device__ __forceinline__ StackT(int* lds_column, uint32_t* spill_area, uint32_t spill_depth, int sp0)
      : lds((LdsIntPtr)lds_column), spill(reinterpret_cast<char*>(spill_area)), spill_off(lane_slot() * spill_depth * 4u), sp(sp0) {}
  __device__ __forceinline__ uint32_t* spilt(int level) const { return reinterpret_cast<uint32_t*>(spill + (spill_off + ((uint32_t)(level - kLevels) << 2))); }
  __device__ __forceinline__ void push(int v) {
    if (sp < kLevels) lds[sp * kBlock] = v; else *spilt(sp) = (uint32_t)v;
    ++sp;
  }
  __device__ __forceinline__ int pop() {
    --sp;
    int v;
    if (__builtin_expect(sp < kLevels, 1)) v = lds[sp * kBlock]; else v = (int)*spilt(sp);   // two loads of two address spaces: not to be merged
    return v;
  }
  // Hand-overs take the OLDEST live entry of a stack (the lowest level, aux_sb) and move that mark up by one, so the stolen entries are
  // one run at the bottom: a pop that finds kStolen has found the end of the lane's own work -- everything below is stolen as well.
  // (Walking down through the marks one LDS read at a time, as rounds 1-3 did, was most of the 1 100 clocks a node iteration of a small
  // share spent behind its box tests: the whole wave waits while one lane scans.)
  __device__ __forceinline__ int pop_live() {
    if (sp > 0) {
      const int v = pop();
      if (v != kStolen) return v;
      sp = 0;
    }
    return kRayDone;
  }
};
using Stack = StackT<kLdsStack>;
constexpr int kLdsStack8 = GLZ_TRACE8_STACK;   // LDS levels of the 8-wide tracer's stacks (a visit pushes up to seven; its blocks run four to a CU: 28 KB + 8 KB of scratch each)

struct TraceTally {
  unsigned long long rays = 0, nodes = 0, tris = 0, hits = 0, fresh = 0;
  // phase occupancy (instrumented build only): rounds executed and lanes doing useful work in them, counted on lane 0
  unsigned long long node_iters = 0, node_lanes = 0, leaf_iters = 0, leaf_lanes = 0, refill_iters = 0, refill_lanes = 0;
};

// ---------------------------------------------------------------------------------------------
// Wave-persistent traversal.  A wave owns a strided sequence of 64-ray groups (group g of wave w is rays
// [64 * (g * n_waves + w), +64)) and keeps its 64 lanes busy: a lane whose ray has finished takes the next
// ray of the wave's sequence as soon as kRefill lanes are idle (no atomics: the sequence pointer is wave
// uniform).  Each round is  [refill] -> [inner-node phase, a share step before each of its iterations] -> [leaf phase] -> [merge] -> [retire]:
//   * inner-node phase: lanes sitting on an inner node test its four child boxes, descend into the nearest
//     hit child and push the others farthest first; lanes that reached a leaf wait.  The phase ends when no lane is on an
//     inner node, or when at least kLeafQuorum lanes are waiting on a leaf.
//     A lane with an ANY-HIT ray does the opposite (GLZ_ANY_FAR_FIRST): it descends into the hit child with the LARGEST entry distance and
//     pushes the others nearest first, so that the next-farthest is popped next.  Nearest first is the order for finding the nearest hit; a
//     shadow ray only has to find one, and what occludes it in a scene with walls and a roof stands at its far end -- the small boxes
//     around the surface it leaves almost never do (tools/bvh_lab anyorder=: 15.6 -> 10.6 node visits, 2.02 -> 1.13 leaf visits per shadow
//     ray of the bench scene).  The counting kernels walk both kinds nearest first: their counts are defined by the oracle's walk.
//   * leaf phase: every lane on a leaf runs the exact ray/triangle test once, then pops its stack.
//   * share / merge (only once the wave's sequence is exhausted, i.e. in the tail): an idle lane takes the OLDEST
//     pending subtree off the LDS stack of a busy lane (the stacks are LDS columns, so any lane can reach them),
//     copies that lane's ray through shuffles and traverses the subtree as a helper; its result is merged back into
//     the owner (smaller t, then smaller world id; any hit for shadow rays), which retires when no helper is left.  Owner and
//     helpers prune with the closest distance any of them has found so far (aux_t).
//     The longest rays then finish in a fraction of their serial time: they set the duration of a launch once a GPU
//     holds few rays per wave (tile sharding over 8 GPUs: k_trace's floor was 0.17 ms whatever the share of the frame).
//     Closest-hit and any-hit results do not depend on the visit order, so sharing changes no result; it is compiled
//     out of the instrumented kernels, whose node / triangle counts are defined by the serial walk.
// This replaces the one-ray-per-thread loop whose VALU lane utilisation was 24 % on the atrium
// (SQ_THREAD_CYCLES_VALU / (64 * SQ_ACTIVE_INST_VALU), profiles/r01b_sq_counters.txt).
//
// ANY = false: closest hit in (tmin, tmax); ties on t go to the smaller world triangle id, so the result
// does not depend on visit order.  ANY = true: the first accepted hit ends the ray.
// Source: bool load(uint32_t ray, vec3& o, vec3& d, float& tmin, float& tmax)   (false = nothing to trace or report)
// Sink:   void store(uint32_t ray, const HitRecord&)
// lds_col: this lane's stack column; aux: this WAVE's 3 x 64 ints of LDS scratch (helpers per owner, donor list, stack bottoms)
// ---------------------------------------------------------------------------------------------
// (thresholds: device/tuning.h.  Leaf quorum: 12 / 16 / 20 / 24 / 32 lanes -> 0.571 / 0.554 / 0.542 / 0.541 / 0.557 ms per k_trace;
// the tail of a small share and the shadow rays have the same optimum.)
constexpr int kRefill = GLZ_REFILL;
constexpr int kTlRefill = GLZ_TL_REFILL;
constexpr int kLeafQuorum = GLZ_LEAF_QUORUM;
constexpr int kRefillAny = GLZ_REFILL_ANY, kLeafQuorumAny = GLZ_LEAF_QUORUM_ANY;   // the same for a pass of shadow rays only (k_trace's second pass, its shadow waves)
constexpr int kAlphaQuorum = GLZ_ALPHA_QUORUM;   // lanes waiting for the alpha test at which the alpha phase runs (trace_wave)
constexpr int kAuxPerWave = 3 * 64 + 4 * 64;   // work sharing (3 x 64) + the four child links of the node a lane is visiting
// The block's scratch, as the kernels declare it (__shared__ alignas(1024) int s_aux[kAuxPerBlock]): the waves' link areas first -- 256 ints
// each, so that every one of them starts on a 1 KB boundary (sorted_link) -- then their work-sharing words.
constexpr int kAuxPerBlock = (kBlock / 64) * kAuxPerWave;
__device__ __forceinline__ int* wave_links(int* s_aux, uint32_t wave_in_block) { return s_aux + 256u * wave_in_block; }
__device__ __forceinline__ int* wave_aux(int* s_aux, uint32_t wave_in_block) { return s_aux + 256u * (kBlock / 64) + 192u * wave_in_block; }

// The SIMD issues its OLDEST ready wave first, and the tracers are bound by VALU issue: with one priority for all, the waves of the
// blocks dispatched first ran 1.6 x faster than the last ones' through the same amount of work (1.67 against 2.66 us per node
// iteration) and then sat idle while those finished -- the closest-hit phase of a full frame ended between 240 and 396 us
// (tools/gpu_wave_times.py, by position in the grid, not by XCD).  Every wave changes its issue priority once per round, starting from
// the sixth of the grid its block is in: all get the same share, the phase ends between 307 and 389 us, k_trace 0.540 -> 0.514 ms
// (only for shares that give a wave at least two whole groups, see `rotate` in trace_wave).
// (Per node iteration instead of per round, keyed by the hardware wave slot instead of the block index, every second round: the
// same; every fourth round 0.523; priority by the wave's own progress -- groups behind first -- 0.545; the youngest first 0.566.)
// Six waves per SIMD, four levels: a cycle of six turns 3 2 2 1 1 0 (with four turns, waves four apart always tie and the older one wins: 0.514 -> 0.509 ms).
__device__ __forceinline__ void rotate_priority(uint32_t turn) {
  const uint32_t p = turn & 3u;   // s_setprio takes an immediate
  if (p == 0u) __builtin_amdgcn_s_setprio(0); else if (p == 1u) __builtin_amdgcn_s_setprio(1); else if (p == 2u) __builtin_amdgcn_s_setprio(2); else __builtin_amdgcn_s_setprio(3);
}

// the link of the child a sort key names, out of the wave's link scratch (`base` = LDS byte address of this lane's word of child 0, bits 8..9 zero)
__device__ __forceinline__ int sorted_link(uint32_t base, uint32_t key) {
  return *(LdsIntPtr)(uintptr_t)((key & kKeyChildMask) | base);
}

// The staged nodes are read through a pointer that keeps its LDS address space: with a generic pointer the compiler
// merges the LDS and the global fetch of a node into ONE flat_load behind a pointer select -- every node of the tree then
// comes in through the flat path (measured: k_trace 0.586 -> 0.786 ms).
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef const __attribute__((address_space(3))) u32x4* LdsNodePtr;

// The rays a wave works through, in the order it takes them (all wave-uniform but the position asked for): the 64-ray groups are
// dealt round-robin, group g to wave g % n_waves.  (Dealing the left-over rays in pieces smaller than a group, so that every wave gets
// the same share of them, is slower everywhere -- a wave's iteration costs the same whatever the number of its lanes that work:
// EXPERIMENTS.md.)
struct RaySequence {
  uint32_t wave, n_waves, total;
  uint32_t own_full;     // rays this wave takes in whole rounds of the deal (a last, partial round may add one more group)
  __device__ __forceinline__ RaySequence(uint32_t wave_, uint32_t n_waves_, uint32_t total_) : wave(wave_), n_waves(n_waves_), total(total_) {
    own_full = (((total + 63u) >> 6) / n_waves) * 64u;
  }
  // ray at position `pos` of this wave's sequence; >= total: the sequence has ended (ray_at is monotonic in pos)
  // (A wave's groups neighbours of EACH OTHER -- groups 6 w .. 6 w + 5 -- instead of its block-mates': k_trace 0.510 -> 0.561 ms.)
  __device__ __forceinline__ uint32_t ray_at(uint32_t pos) const { return (wave + (pos >> 6) * n_waves) * 64u + (pos & 63u); }
};

#ifdef GLZ_SECTION_TIMES   // tuning builds only (tools/gpu_sections.py): shader clocks every wave spent in each part of trace_wave's round, and how often
static __device__ unsigned long long g_sections[16 * 8192];   // per wave: clocks {refill, share, node visit, loop control, leaf, merge + retire}, counts {rounds, node iterations, leaf phases, hand-over steps with a taker}
#define GLZ_SEC_STAMP(acc) do { const unsigned long long now_ = __builtin_amdgcn_s_memtime(); (acc) += now_ - sec_t; sec_t = now_; } while (0)
#else
#define GLZ_SEC_STAMP(acc) do { } while (0)
#endif
#ifdef GLZ_WAVE_TIMES
__device__ unsigned long long g_wave_times[3 * 8192];
__device__ unsigned int g_wave_stats[8 * 8192];   // closest-hit phase: rounds, node iterations, lanes in them, leaf iterations, lanes in them, rounds with helpers
__device__ unsigned long long g_tl_stats[8];      // two-level tracer, summed over lanes: rays, top-level node visits, mesh node visits, instances entered, triangle tests, node iterations, leaf iterations
#endif

// MIXED (with ANY = false): the sequence holds rays of both kinds, the source says which after every load (src.any) -- k_path
// traces a wave's closest-hit rays and the shadow rays its previous launch queued in ONE pass, the shadow rays in the lanes
// the closest-hit rays leave idle.
// PREFETCH (k_path): the four 16-byte loads of a lane's NEXT inner node are issued the moment the node is known -- at the end of the visit
// that chose it, after a leaf phase's pop, when an idle lane takes a subtree over -- instead of at the top of the next node iteration, so
// that they are in flight during the pushes, the loop's ballots and the hand-overs to idle lanes in between.  A small share of the frame is
// bound by the LATENCY of this dependent chain (tools/gpu_sections.py: a node visit of a 1/32 share, on an otherwise idle chip, still takes
// 1 800 clocks, most of them waiting for the node), not by issue; the full-frame k_trace is issue bound and has no 16 registers to spare.
// WIDE8 (k_trace8, the tracer of a small tile share): the hierarchy's 8-wide nodes (types.h BvhNode8, two lines a visit).  A GPU that holds
// one 64-ray group per resident wave is bound by the LATENCY of a ray's chain of dependent node fetches (1 800 - 2 100 clocks per node
// iteration whatever the load), and eight-wide that chain is 31 % shorter (17.3 against 24.9 visits per sample on the bench scene,
// tools/bvh_lab); the full frame is bound by VALU issue and by the address units, where twice the boxes per visit cost more than the
// visits saved (it keeps the 4-wide nodes).  The nearest child is entered (the farthest in its pass of any-hit rays), the others are pushed in slot order -- no sort: ordering the
// rest by distance as well saves 0.7 % of the visits (tools/bvh_lab order=nearest) for 38 instructions a visit; the child links are
// picked in registers (a select tree on the key's child bits) rather than through LDS, one round trip less on the chain.  Hits do not
// depend on the visit order, so the images are those of the 4-wide walk bit for bit.  No staged top (the root is node 0), a deeper LDS
// stack (kLdsStack8).
// ALPHA: what becomes of a candidate on non-opaque geometry -- kAlphaNone: the scene has none (DeviceScene::has_non_opaque == 0; the
// kernel carries no alpha code), kAlphaInline: tested where it is met (the counting kernels, whose fetch counts are defined by the
// serial walk; k_path; k_trace8), kAlphaPhase: it waits for an alpha phase of its own (k_trace for scenes with opacity maps).
constexpr int kAlphaNone = 0, kAlphaInline = 1, kAlphaPhase = 2;
template <bool ANY, bool COUNT, bool MIXED = false, bool PREFETCH = false, bool WIDE8 = false, int ALPHA = kAlphaInline, class Source, class Sink>
__device__ __forceinline__ void trace_wave(const DeviceScene& S, Source& src, Sink& sink, int* __restrict__ lds_col, int* aux, int* link_scratch, LdsNodePtr top_lds,
                                           uint32_t* __restrict__ spill, uint32_t spill_depth, uint32_t total, uint32_t wave, uint32_t n_waves, TraceTally& tally) {
  constexpr bool SHARE = !COUNT;
  constexpr bool TOP = !WIDE8;   // the top kBvhTopNodes nodes of the tree come from a per-block LDS copy ("LDS-staged node packets", stage_top)
  constexpr int kLevels = WIDE8 ? kLdsStack8 : kLdsStack;
  // the order of a node's children (box_key): any-hit rays farthest first, per pass where the pass has one kind of ray, per lane in a MIXED pass
  constexpr bool FAR = GLZ_ANY_FAR_FIRST != 0 && (!COUNT || GLZ_COUNT_ANY_FAR_FIRST != 0);
  constexpr int ORDER = !FAR ? kKeysNearFirst : (ANY ? kKeysFarFirst : (MIXED ? kKeysPerLane : kKeysNearFirst));
  static_assert(!(WIDE8 && MIXED), "the 8-wide walk picks its first child per pass");
  constexpr uint32_t kMiss = kKeyMiss<ORDER>;
  const BvhNode8* __restrict__ nodes8 = S.bvh_nodes8;
  constexpr uint32_t kNone = 0xFFFFFFFFu;
  // The wave's place in the deal is the same in all of its lanes, and the compiler has to KNOW that: everything that steers the rounds below
  // (`seq`, `exhausted`, the loops' exits) derives from these three, and a build in which they arrived through variables the compiler
  // could not prove uniform turned the loops into divergent ones -- lanes "leave" one by one, EXEC is empty behind the last exit -- and
  // placed the reloads of spilt registers in front of the instruction that restores EXEC: what was kept across the pass came back as
  // whatever the registers held (EXPERIMENTS.md, round 5: a few wrong pixels from run to run; clang 22).  v_readfirstlane says it.
  wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)wave);
  n_waves = (uint32_t)__builtin_amdgcn_readfirstlane((int)n_waves);
  total = (uint32_t)__builtin_amdgcn_readfirstlane((int)total);
  const BvhNode4* __restrict__ nodes = S.bvh_nodes;
  const BvhGrid grid = S.bvh_grid;
  const int lane = threadIdx.x & 63;
  const unsigned long long lanes_below = (1ull << lane) - 1ull;
  int* aux_out = aux;          // [owner lane] helpers currently working for that lane's ray
  uint32_t* aux_t = reinterpret_cast<uint32_t*>(aux) + 64;   // [owner lane] bits of the smallest hit distance the ray's owner or any helper has found (tail only)
  int* aux_sb = aux + 128;     // [lane] lowest LDS stack level that may still hold a live entry
  int* aux_pair = link_scratch;   // [k] lane of the k-th donor of this round; shares its words with the child links, which only live inside a node visit
  if (SHARE) {
    aux_out[lane] = 0;
    aux_sb[lane] = 0;
  }
  uint32_t seq = 0;                                         // wave-uniform: rays of this wave's sequence handed out so far
  const RaySequence rays(wave, n_waves, total);
  // A share of the frame that gives a wave fewer than two whole groups is one long tail (work sharing from the first round on): there
  // the rotation costs 3 % (1/4 share 0.245 -> 0.253 ms per launch, 1/8 0.146 -> 0.150) where the full frame gains 4 % and a half 4.5 %.
  // (Rotating only until the wave's sequence is exhausted gains nothing anywhere: what the rotation evens out is the waves' last groups.)
  const bool rotate = rays.own_full >= 128u;
  // (giving each XCD one contiguous eighth of the groups -- rays of one image band per L2 -- measured 5 % slower: the bands
  // differ in cost and the static split loses more to imbalance than the L2 gains)
  // (Drawing the groups from a counter instead of the stride: the waves of a full-frame launch end between 257 and 406 us of a
  // 410 us closest-hit phase -- 5 or 6 groups each -- tools/gpu_wave_times.py.  One counter: 577 us, device-scope atomics on one
  // address are served at ~15 ns each; 32 interleaved counters: the ends move together, 306 - 400 us, but every wave gets slower --
  // neighbouring groups no longer run on one CU at one time -- 0.572 ms per k_trace either way; whole rounds by the stride and
  // only the last partial round drawn: 0.601 ms.  A wave's last group runs without refills behind it whoever hands it out.)
  bool exhausted = rays.ray_at(0u) >= total;                // wave-uniform
  // per-lane ray state
  bool open = false;                                        // a ray of this lane's own is in flight and its result has not been stored
  bool helper = false;                                      // this lane traverses a subtree of lane `ray`'s ray (work sharing)
  bool found_own = false;                                   // ... and has accepted a hit of its own since it took the subtree over (merge)
  bool any_lane = ANY;                                      // the ray in this lane ends with its first accepted hit (MIXED: per ray)
  bool alpha_wait = false;                                  // the lane sits on a leaf (cur < 0) with a candidate that needs the alpha test: it waits for the alpha phase
  int cur = kRayDone;
  uint32_t ray = 0;                                         // ray index (open) or owner lane (helper)
  vec3 o = mk3(0.0f, 0.0f, 0.0f), d = mk3(0.0f, 0.0f, 1.0f);
  vec3 ig = mk3(0.0f, 0.0f, 0.0f), cg = mk3(0.0f, 0.0f, 0.0f);   // grid-space ray: plane q is crossed at t = q * ig + cg
  SlabSel sel{kSlabSelLo, kSlabSelLo, kSlabSelLo};             // near-plane selectors, from the signs of ig
  float tmin = 0.0f, tmax = 0.0f;
  HitRecord best{0.0f, 0.0f, 0.0f, kNone};
  uint32_t best_id = kNone;
  // the spill area is indexed by the physical lane slot of the grid (lane_slot)
  StackT<kLevels> st{lds_col, spill, spill_depth, 0};
  // PREFETCH: the node `pf_cur` as loaded (or on its way)
  u32x4 pf0 = {0u, 0u, 0u, 0u}, pf1 = pf0, pf2 = pf0, pf3 = pf0, pf4 = pf0, pf5 = pf0, pf6 = pf0, pf7 = pf0;
  int pf_cur = -1;
  auto prefetch_node = [&]() {
    if (PREFETCH && WIDE8 && cur >= 0 && cur < kStolen) {
      const u32x4* np = reinterpret_cast<const u32x4*>(record_at(nodes8, (uint32_t)cur));
      pf0 = np[0]; pf1 = np[1]; pf2 = np[2]; pf3 = np[3]; pf4 = np[4]; pf5 = np[5]; pf6 = np[6]; pf7 = np[7];
      pf_cur = cur;
    } else
    if (PREFETCH && !WIDE8 && cur >= 0 && !(cur & kBvhTopFlag)) {   // a node of the table in memory (staged nodes, kRayDone and kStolen carry bit 30)
      const u32x4* np = reinterpret_cast<const u32x4*>(record_at(nodes, (uint32_t)cur));
      pf0 = np[0]; pf1 = np[1]; pf2 = np[2]; pf3 = np[3];
      pf_cur = cur;
    }
    // (The 64-byte record of a LEAF requested the same way, while the lane waits for the leaf phase's quorum: slower, a 1/8 share
    // 0.1379 -> 0.1418 ms per launch, 1/16 0.0997 -> 0.1058.)
  };
#ifdef GLZ_WAVE_TIMES
  unsigned int wt_rounds = 0, wt_node_iters = 0, wt_node_lanes = 0, wt_leaf_iters = 0, wt_leaf_lanes = 0, wt_helper_rounds = 0, wt_wait_rounds = 0;
#endif
#ifdef GLZ_SECTION_TIMES
  unsigned long long sec_t = __builtin_amdgcn_s_memtime(), sec_refill = 0, sec_share = 0, sec_node = 0, sec_ctl = 0, sec_leaf = 0, sec_tail = 0;
  unsigned long long sec_rounds = 0, sec_iters = 0, sec_leaves = 0, sec_takes = 0, sec_merges = 0, sec_merge = 0, sec_f0 = 0, sec_f1 = 0, sec_f2 = 0;
#endif
  // issue-priority rotation (rotate_priority above); k_path's MIXED pass keeps the priority its own kernel set
  // (inside k_path's mixed pass as well: a 1/4 share 0.276 -> 0.263 ms per launch, 1/8 0.1456 -> 0.1449, 1/16 0.118 -> 0.123)
  constexpr bool ROTATE = !MIXED;
  const uint32_t prio_gen = (blockIdx.x * 6u) / gridDim.x;   // which sixth of the grid: the order the blocks of a CU were dispatched in
  uint32_t prio_round = 0;
  // ---- share: idle lanes adopt the oldest pending subtree of a busy lane (called before every node iteration, see below) ----
  auto share_step = [&]() {
  if (SHARE && exhausted)
  for (int rep = 0; rep < 1; ++rep) {   // (more than one hand-over per donor and node iteration costs more in shuffles than it gains: 0.145 / 0.148 / 0.152 ms for 1 / 2 / 3)
    bool more = false;
    const bool busy = open || helper;
    const unsigned long long idle_m = __ballot(!busy);
    if (idle_m != 0ull) {
      if (ANY || MIXED) {   // helpers of a ray whose hit has been found have nothing left to decide
        const int owner_found = __shfl((int)(best.leaf != kNone), helper ? (int)ray : lane);
        if (helper && any_lane && owner_found) cur = kRayDone;
      }
      int sb = 0, lim = 0;
      if (busy && cur != kRayDone) {
        sb = aux_sb[lane];
        if (sb > st.sp) sb = st.sp;
        lim = st.sp < kLevels ? st.sp : kLevels;
        while (sb < lim && st.lds[sb * kBlock] == kStolen) ++sb;
        aux_sb[lane] = sb;
      }
      const bool can_give = busy && cur != kRayDone && sb < lim;
      const unsigned long long give_m = __ballot(can_give);
      const int n_give = __popcll(give_m), n_take = __popcll(idle_m);
      const int n_pairs = n_give < n_take ? n_give : n_take;
      if (n_pairs > 0) {
        int give = 0;
        if (can_give && __popcll(give_m & lanes_below) < n_pairs) {
          give = st.lds[sb * kBlock];
          st.lds[sb * kBlock] = kStolen;
          aux_sb[lane] = sb + 1;
          aux_pair[__popcll(give_m & lanes_below)] = lane;
        }
        const int take_rank = __popcll(idle_m & lanes_below);
        const bool take = !busy && take_rank < n_pairs;
        const int donor = take ? aux_pair[take_rank] : lane;   // same-wave LDS: the stores above are complete (in-order)
        // Every lane runs the shuffles.  Lanes that take nothing read their own lane (donor == lane), so the ray registers
        // can be assigned unconditionally: no temporaries stay live across the block (register pressure: 72 VGPRs).
        const int t_node = __shfl(give, donor);
        const int t_owner = __shfl(helper ? (int)ray : lane, donor);
        o.x = __shfl(o.x, donor); o.y = __shfl(o.y, donor); o.z = __shfl(o.z, donor);
        d.x = __shfl(d.x, donor); d.y = __shfl(d.y, donor); d.z = __shfl(d.z, donor);
        ig.x = __shfl(ig.x, donor); ig.y = __shfl(ig.y, donor); ig.z = __shfl(ig.z, donor);
        cg.x = __shfl(cg.x, donor); cg.y = __shfl(cg.y, donor); cg.z = __shfl(cg.z, donor);
        sel = SlabSel{slab_sel(ig.x), slab_sel(ig.y), slab_sel(ig.z)};
        tmin = __shfl(tmin, donor); tmax = __shfl(tmax, donor);
        best.t = __shfl(best.t, donor); best.u = __shfl(best.u, donor); best.v = __shfl(best.v, donor);
        best.leaf = (uint32_t)__shfl((int)best.leaf, donor);
        best_id = (uint32_t)__shfl((int)best_id, donor);
        if (MIXED) any_lane = __shfl((int)any_lane, donor) != 0;
#ifdef GLZ_SECTION_TIMES
        sec_takes += 1;
#endif
        if (take) {
          ray = (uint32_t)t_owner;
          cur = t_node;
          st.sp = 0;
          aux_sb[lane] = 0;
          helper = true;
          found_own = false;
          alpha_wait = false;
          atomicAdd(&aux_out[t_owner], 1);
          prefetch_node();
        }
        more = n_take > n_give;   // idle lanes are left over: the donors may have more to give
      }
    }
    if (!more) break;
  }
  };
  for (;;) {
#ifdef GLZ_WAVE_TIMES
    wt_rounds += 1;
    wt_helper_rounds += __ballot(helper) != 0ull;
    wt_wait_rounds += __ballot(open && cur == kRayDone) != 0ull && __ballot(open && cur != kRayDone) == 0ull;   // owners only waiting for helpers
#endif
    if (ROTATE && rotate) {   // six waves per SIMD, four levels: a cycle of six turns 3 2 2 1 1 0
      const uint32_t pos = (prio_gen + prio_round++) % 6u;
      rotate_priority(pos == 0u ? 3u : (pos < 3u ? 2u : (pos < 5u ? 1u : 0u)));
    }
#ifdef GLZ_SECTION_TIMES
    sec_rounds += 1;
#endif
    GLZ_SEC_STAMP(sec_tail);
    // ---- refill ----
    const unsigned long long idle = __ballot(!(open || helper));
    const int n_idle = __popcll(idle);
    if (!exhausted && n_idle >= (ANY ? kRefillAny : kRefill)) {
      if (COUNT && lane == 0) { tally.refill_iters += 1; tally.refill_lanes += (unsigned)n_idle; }
      const uint32_t next_ray = rays.ray_at(seq + (uint32_t)__popcll(idle & lanes_below));
      if (!open && next_ray < total) {
        if (src.load(next_ray, o, d, tmin, tmax)) {
          ray = next_ray;
          alpha_wait = false;
          best = HitRecord{tmax, 0.0f, 0.0f, kNone};
          best_id = kNone;
          if constexpr (MIXED) any_lane = src.any;
          if (COUNT) tally.rays += 1;
          if (S.n_world_tris == 0 || !ray_is_finite(o, d)) {
            sink.store(ray, best);                          // nothing to intersect / nothing can be hit: a miss
          } else {
            const vec3 og = mk3((o.x - grid.lo[0]) * grid.inv_cell[0], (o.y - grid.lo[1]) * grid.inv_cell[1], (o.z - grid.lo[2]) * grid.inv_cell[2]);
            if (COUNT) ig = mk3(grid_inv_dir(d.x) * grid.cell[0], grid_inv_dir(d.y) * grid.cell[1], grid_inv_dir(d.z) * grid.cell[2]);
            else ig = mk3(grid_inv_dir_fast(d.x) * grid.cell[0], grid_inv_dir_fast(d.y) * grid.cell[1], grid_inv_dir_fast(d.z) * grid.cell[2]);
            cg = mk3(grid_addend(og.x, ig.x), grid_addend(og.y, ig.y), grid_addend(og.z, ig.z));
            sel = SlabSel{slab_sel(ig.x), slab_sel(ig.y), slab_sel(ig.z)};
            st.sp = 0;
            if (SHARE) aux_sb[lane] = 0;
            cur = TOP ? kBvhTopFlag : 0;   // the root (slot 0 of the staged table)
            open = true;
          }
        }
      }
      seq += (uint32_t)n_idle;
      exhausted = rays.ray_at(seq) >= total;
      // The tail begins: from here on a ray may be worked on by several lanes, which tell each other the closest distance found so
      // far through aux_t -- a helper walking a far subtree with the bound it was handed at the start would go through all of
      // it after the owner has long found something nearer, and the owner cannot retire before its helpers are back.
      if (SHARE && !ANY && exhausted && open) aux_t[lane] = __float_as_uint(best.t);
    }
    GLZ_SEC_STAMP(sec_refill);
    if (__ballot(open || helper) == 0ull) {
      if (exhausted) break;
      continue;
    }
    // ---- inner-node phase ----
    for (;;) {
      // Idle lanes take over pending subtrees before EVERY node iteration of the tail, not once per round: a round is several
      // iterations long, and with one hand-over per round the helpers of a long ray multiplied too slowly to matter before it
      // was over (a 1/8 share: 0.153 -> 0.147 ms per launch; the full frame, where only each wave's last group is a tail: 0.930 -> 0.914).
      // (Every 2nd / 3rd node iteration instead: a 1/8 share 0.1352 -> 0.1382 / 0.1404 ms per launch.)
      GLZ_SEC_STAMP(sec_ctl);
      share_step();
      GLZ_SEC_STAMP(sec_share);
      // (Reading the first word of the triangle as soon as a lane of the tail arrives at a leaf, so that the line is on its way while
      // the others finish their node iterations: slower, 0.146 -> 0.149 ms for a 1/8 share and 0.905 -> 0.924 ms for the full frame.)
      const bool at_node = cur >= 0 && cur < kStolen;
      const unsigned long long m_node = __ballot(at_node);
      if (m_node == 0ull) break;
      if (COUNT && lane == 0) { tally.node_iters += 1; tally.node_lanes += (unsigned)__popcll(m_node); }
#ifdef GLZ_WAVE_TIMES
      wt_node_iters += 1; wt_node_lanes += (unsigned)__popcll(m_node);
#endif
#ifdef GLZ_SECTION_TIMES
      sec_iters += 1;
#endif
      GLZ_SEC_STAMP(sec_ctl);
      if (WIDE8) {
       if (at_node) {
        // 128-byte node = 8 x dwordx4: eight child boxes and eight links.  The nearest child is entered, the others pushed in slot order.
        u32x4 w0, w1, w2, w3, w4, w5, w6, w7;
        if (PREFETCH) {
          if (pf_cur != cur) prefetch_node();
          w0 = pf0; w1 = pf1; w2 = pf2; w3 = pf3; w4 = pf4; w5 = pf5; w6 = pf6; w7 = pf7;
        } else {
          const u32x4* np = reinterpret_cast<const u32x4*>(record_at(nodes8, (uint32_t)cur));
          w0 = np[0]; w1 = np[1]; w2 = np[2]; w3 = np[3]; w4 = np[4]; w5 = np[5]; w6 = np[6]; w7 = np[7];
        }
        if (COUNT) tally.nodes += 1;
        float bound = best.t;
        if (SHARE && !ANY && exhausted) bound = fminf(bound, __uint_as_float(aux_t[helper ? (int)ray : lane]));
        uint32_t key[8];
        constexpr bool FAR8 = ORDER == kKeysFarFirst;   // a pass of any-hit rays: the child entered is the farthest (a max tree, misses are 0), the rest keep slot order
        key[0] = box_key8<FAR8>(w0.x, w0.y, w0.z, 0u << 8, sel, ig, cg, tmin, bound); key[1] = box_key8<FAR8>(w0.w, w1.x, w1.y, 1u << 8, sel, ig, cg, tmin, bound);
        key[2] = box_key8<FAR8>(w1.z, w1.w, w2.x, 2u << 8, sel, ig, cg, tmin, bound); key[3] = box_key8<FAR8>(w2.y, w2.z, w2.w, 3u << 8, sel, ig, cg, tmin, bound);
        key[4] = box_key8<FAR8>(w3.x, w3.y, w3.z, 4u << 8, sel, ig, cg, tmin, bound); key[5] = box_key8<FAR8>(w3.w, w4.x, w4.y, 5u << 8, sel, ig, cg, tmin, bound);
        key[6] = box_key8<FAR8>(w4.z, w4.w, w5.x, 6u << 8, sel, ig, cg, tmin, bound); key[7] = box_key8<FAR8>(w5.y, w5.z, w5.w, 7u << 8, sel, ig, cg, tmin, bound);
        auto first_of = [](uint32_t a, uint32_t b) { return (FAR8 ? a > b : a < b) ? a : b; };
        const uint32_t ka = first_of(key[0], key[1]), kb = first_of(key[2], key[3]), kc = first_of(key[4], key[5]), kd = first_of(key[6], key[7]);
        const uint32_t kab = first_of(ka, kb), kcd = first_of(kc, kd);
        const uint32_t kmin = first_of(kab, kcd);   // the key of the child to enter
        if (kmin == kMiss) {
          cur = SHARE ? st.pop_live() : (st.sp ? st.pop() : kRayDone);
          prefetch_node();
        } else {
          const int link[8] = {(int)w6.x, (int)w6.y, (int)w6.z, (int)w6.w, (int)w7.x, (int)w7.y, (int)w7.z, (int)w7.w};
          const bool b0 = (kmin & 0x100u) != 0u, b1 = (kmin & 0x200u) != 0u, b2 = (kmin & 0x400u) != 0u;
          const int s01 = b0 ? link[1] : link[0], s23 = b0 ? link[3] : link[2], s45 = b0 ? link[5] : link[4], s67 = b0 ? link[7] : link[6];
          const int t03 = b1 ? s23 : s01, t47 = b1 ? s67 : s45;
          const int entered = b2 ? t47 : t03;
          if (__ballot(st.sp + 7 > kLevels) == 0ull) {   // wave-uniform: every lane stays inside the LDS part of its stack
#pragma unroll
            for (int k = 7; k >= 0; --k)
              if (key[k] != kMiss && key[k] != kmin) { st.lds[st.sp * kBlock] = link[k]; ++st.sp; }
          } else {
#pragma unroll
            for (int k = 7; k >= 0; --k)
              if (key[k] != kMiss && key[k] != kmin) st.push(link[k]);
          }
          cur = entered;
          prefetch_node();
        }
       }
      } else
      if (at_node) {
        // 64-byte node = 4 x dwordx4: four child boxes in 16-bit grid coordinates (the ray was mapped into grid units at
        // refill) and four links.  Children are entered nearest first; the others are pushed farthest first (any-hit rays: the reverse).
        // Nodes of the top levels come out of the block's LDS copy (their `cur` carries kBvhTopFlag | slot); lanes that read the
        // same staged node broadcast.
        u32x4 w0, w1, w2, w3;
        if (TOP && (cur & kBvhTopFlag)) {
          LdsNodePtr np = top_lds + 4 * (cur & 0xFFFF);
          w0 = np[0]; w1 = np[1]; w2 = np[2]; w3 = np[3];
        } else if (PREFETCH) {
          if (pf_cur != cur) prefetch_node();   // (the ray has just started, or its stack was popped by someone who could not know)
          w0 = pf0; w1 = pf1; w2 = pf2; w3 = pf3;
        } else {
          const u32x4* np = reinterpret_cast<const u32x4*>(record_at(nodes, (uint32_t)cur));
          w0 = np[0]; w1 = np[1]; w2 = np[2]; w3 = np[3];
          // (A fifth 16-byte load from the node's own line costs 2.4 % of the kernel, 0.580 -> 0.594 ms: a 48-byte node format --
          // 8-bit boxes relative to a per-node origin -- would buy about that and pay ~12 VALU instructions per visit for it.)
        }
        if (COUNT) tally.nodes += 1;
#if defined(GLZ_SECTION_TIMES) && GLZ_SECTION_TIMES >= 2   // -DGLZ_SECTION_TIMES=2: the node visit in pieces
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        GLZ_SEC_STAMP(sec_f0);   // the node's words are here
#endif
        float bound = best.t;
        if (SHARE && !ANY && exhausted) bound = fminf(bound, __uint_as_float(aux_t[helper ? (int)ray : lane]));   // positive floats order like their bits
        // (k0 .. k3 sorted: the child to enter, then the others in the order they are to be popped -- by distance from the near end, for any-hit
        // rays from the far end: box_key's ORDER)
        const uint32_t flip = (ORDER == kKeysPerLane && any_lane) ? kKeyDistanceMask : 0u;
        uint32_t k0 = box_key<false, ORDER>(w0.x, w0.y, w0.z, w3.x, 0u, sel, ig, cg, cg, tmin, bound, flip), k1 = box_key<false, ORDER>(w0.w, w1.x, w1.y, w3.y, kKeyChild, sel, ig, cg, cg, tmin, bound, flip);
        uint32_t k2 = box_key<false, ORDER>(w1.z, w1.w, w2.x, w3.z, 2u * kKeyChild, sel, ig, cg, cg, tmin, bound, flip), k3 = box_key<false, ORDER>(w2.y, w2.z, w2.w, w3.w, 3u * kKeyChild, sel, ig, cg, cg, tmin, bound, flip);
        constexpr bool DESC = ORDER == kKeysFarFirst;
        // (seven instructions, device/sort4.h.  The five-exchange network this replaces cost ten; both leave the keys' VALUES in order, so they
        // agree wherever the keys differ -- hit children always do, by their child bits -- and several miss markers, equal, end up together at
        // the far end either way: nothing downstream tells one miss marker from another.)
        sort4<DESC>(k0, k1, k2, k3);
        // The links go through LDS: picking one of four registers by a per-lane index costs 6 VALU instructions (the
        // kernel's bottleneck), an LDS read at a computed address 2 (k_trace 0.714 -> 0.691 ms).  The scratch is laid out
        // [child][lane] so that every access of a wave instruction has bank = lane % 32 (the [lane][child] layout with one
        // 16-byte store put lanes l, l + 8, l + 16, l + 24 of a half-wave on the same banks: 4.6 M conflict cycles per launch,
        // 22 % of the LDS-active cycles), and all four sorted links are fetched before the first one is used: the reads
        // are independent, so one LDS round trip covers them instead of one per push (read -> wait -> write, four times over).
#if defined(GLZ_SECTION_TIMES) && GLZ_SECTION_TIMES >= 2   // -DGLZ_SECTION_TIMES=2: the node visit in pieces
        asm volatile("" : "+v"(k0), "+v"(k1), "+v"(k2), "+v"(k3));
        GLZ_SEC_STAMP(sec_f1);   // box tests and sort
#endif
        int* links = link_scratch + lane;
        links[0] = (int)w3.x; links[64] = (int)w3.y; links[128] = (int)w3.z; links[192] = (int)w3.w;
        const uint32_t link_base = (uint32_t)(uintptr_t)(LdsIntPtr)links;   // the wave's area is 1 KB aligned: bits 8..9 are the child's
        const int l0 = sorted_link(link_base, k0), l1 = sorted_link(link_base, k1), l2 = sorted_link(link_base, k2), l3 = sorted_link(link_base, k3);
        // (Three unconditional stores with the stack pointer advancing by one per valid key -- the invalid links of the sorted
        // sequence are overwritten by the next store or stay above the top -- remove 12 scalar / branch instructions per round
        // and measured slower, 0.587 -> 0.597 ms: the extra DS stores cost more than the exec-mask branches.)
#if defined(GLZ_SECTION_TIMES) && GLZ_SECTION_TIMES >= 2   // -DGLZ_SECTION_TIMES=2: the node visit in pieces
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        GLZ_SEC_STAMP(sec_f2);   // links through LDS
#endif
        if (k0 == kMiss) {
          cur = SHARE ? st.pop_live() : (st.sp ? st.pop() : kRayDone);
          prefetch_node();
        } else {
          if (__ballot(st.sp + 3 > kLdsStack) == 0ull) {   // wave-uniform: every lane stays inside the LDS part of its stack (no spill branches)
            if (k3 != kMiss) { st.lds[st.sp * kBlock] = l3; ++st.sp; }
            if (k2 != kMiss) { st.lds[st.sp * kBlock] = l2; ++st.sp; }
            if (k1 != kMiss) { st.lds[st.sp * kBlock] = l1; ++st.sp; }
          } else {
            if (k3 != kMiss) st.push(l3);
            if (k2 != kMiss) st.push(l2);
            if (k1 != kMiss) st.push(l1);
          }
          cur = l0;
          prefetch_node();
        }
      }
#ifdef GLZ_SECTION_TIMES
      if (!PREFETCH) asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");   // the visit's loads and LDS traffic are charged to the visit
#endif
      GLZ_SEC_STAMP(sec_node);
      if (__popcll(__ballot(cur < 0 && !(ALPHA == kAlphaPhase && alpha_wait))) >= (ANY ? kLeafQuorumAny : kLeafQuorum)) break;
      // (Postponed leaves -- a lane parks the first leaf it arrives at and goes on with its stack, blocks at the second, the parked
      // leaves are tested first in the next leaf phase; Aila & Laine's speculative traversal -- k_trace 0.512 -> 0.540 ms with the
      // leaf phase at 24 waiting lanes, 0.542 / 0.555 at 16 / 32: the visits made without the parked leaf's bound and the second
      // leaf pass cost more than the fuller node iterations save.)
      // (Leaving for a refill as soon as kRefill finished lanes have piled up, without a leaf phase for the few lanes that wait
      // on a leaf, measured slower: 0.588 -> 0.611 ms, node rounds 41.1 -> 42.1 of 64 lanes.  The idle lanes are not what
      // holds the utilisation down.)
    }
    GLZ_SEC_STAMP(sec_ctl);
#ifdef GLZ_SECTION_TIMES
    sec_leaves += __ballot(cur < 0) != 0ull;
#endif
    // ---- leaf phase ----
    if (COUNT) {
      const unsigned long long m_leaf = __ballot(cur < 0);
      if (lane == 0 && m_leaf) { tally.leaf_iters += 1; tally.leaf_lanes += (unsigned)__popcll(m_leaf); }
    }
#ifdef GLZ_WAVE_TIMES
    { const unsigned long long ml = __ballot(cur < 0); if (ml) { wt_leaf_iters += 1; wt_leaf_lanes += (unsigned)__popcll(ml); } }
#endif
    // Candidates on NON-OPAQUE geometry go through the alpha test (raytrace_hit.rahit:24-39) -- the triangle's texture coordinates, the
    // material's opacity map, its descriptor, four texels: a chain of dependent fetches that the whole wave used to sit through whenever ONE
    // of its lanes met such a candidate (with a twentieth of the rays meeting one, most leaf phases: the Sponza-like atrium's k_trace took
    // 0.72 ms against 0.48 without the opacity maps, tools/gpu_sponza_like.py).  So the test has a phase of its own, with a quorum like the
    // leaf phase's: a lane whose leaf holds such a candidate stays on the leaf (alpha_wait) while the others go on, and the waiting lanes
    // take the test together.  The leaf is then tested again from the start -- same operations, same bits -- so nothing is kept per lane
    // but the flag; the candidates of one ray may be decided in another order than the serial walk's, which changes no result (the closest
    // hit is a minimum over the candidates that pass, ties by world id; an occluded ray is occluded).  The counting kernels keep the serial
    // walk: their texture-fetch counts are defined by it.  Measured on one box (tools/gpu_sponza_variants.py, profiles/r05_alpha_phase.txt):
    // the atrium with opacity maps 0.716 -> 0.670 ms per k_trace (quorum 1 / 4 / 8 / 12 / 16 / 24 / 48: 0.807 / 0.745 / 0.686 / 0.673 / 0.670 /
    // 0.701 / 1.018; with the verdict for free 0.601: what is left are the rays that go on through the holes), and the atrium WITHOUT
    // non-opaque geometry 0.489 -> 0.502 for the two ballots a round and the second copy of the leaf code -- so a scene without opacity
    // maps runs the kernel that has no alpha code at all (kAlphaNone).
    constexpr bool DEFER = ALPHA == kAlphaPhase;
    static_assert(!(COUNT && DEFER), "the counting kernels keep the serial walk");
    auto leaf_visit = [&](auto with_alpha_tag) {
      constexpr bool WITH_ALPHA = decltype(with_alpha_tag)::value;
      // A leaf is one 64-byte record (types.h BvhQuad): one triangle or two that share an edge, tested together (ray_quad).  The
      // candidates are then taken in slot order, the order the 48-byte records were walked in (the alpha test's fetches are counted).
      const uint32_t leaf = (uint32_t)~cur;
      const float4* qp = reinterpret_cast<const float4*>(record_at(S.bvh_quads, leaf));
      const float4 r0 = qp[0], r1 = qp[1], r2 = qp[2], r3 = qp[3];
      const uint32_t id0 = __float_as_uint(r0.w), qflags = __float_as_uint(r2.w), slot0 = __float_as_uint(r3.w);
      const bool pair = (qflags & kTriHasPartner) != 0u;
      if (COUNT) tally.tris += pair ? 2 : 1;
      const RayShear rs = ray_shear(d);   // (kept in registers with the ray instead: fits without spills, 0.555 against 0.552 ms -- no gain)
      const QuadHit qh = ray_quad(rs, r0, r1, r2, r3, pair, o, tmin);
      const uint32_t swapped = (qflags & kQuadSwapped) ? 1u : 0u;
      const bool non_opaque = ALPHA != kAlphaNone && (qflags & kTriNonOpaque) != 0u;
      bool finished = false, wait = false;
#pragma nounroll
      for (uint32_t which = 0; which < 2u; ++which) {   // the leaf's first triangle, then its partner
        const bool is_b = (which ^ swapped) != 0u;
        const float t = is_b ? qh.t[1] : qh.t[0], u = is_b ? qh.u[1] : qh.u[0], v = is_b ? qh.v[1] : qh.v[0];
        if ((is_b ? qh.ok[1] : qh.ok[0]) && t < tmax) {
          const uint32_t wid = id0 + which, slot = slot0 + which;
          const bool better = best.leaf == kNone ? true : (t < best.t || (t == best.t && wid < best_id));
          if (better && non_opaque && !WITH_ALPHA) {
            wait = true;   // decided in the alpha phase
          } else if (better && (!non_opaque || alpha_test(S, slot, u, v))) {
            best = HitRecord{t, u, v, slot};
            best_id = wid;
            found_own = true;
            finished = any_lane;
            if (SHARE && !ANY && exhausted) atomicMin(&aux_t[helper ? (int)ray : lane], __float_as_uint(t));
          }
        }
      }
      if (!WITH_ALPHA && wait) {
        alpha_wait = true;   // stays on the leaf
      } else {
        alpha_wait = false;
        cur = finished ? kRayDone : (SHARE ? st.pop_live() : (st.sp ? st.pop() : kRayDone));
        prefetch_node();
      }
    };
    if (cur < 0 && !(DEFER && alpha_wait)) {
      if constexpr (DEFER) leaf_visit(std::false_type{}); else leaf_visit(std::true_type{});
    }
    if constexpr (DEFER) {
      // ---- alpha phase: when enough lanes wait for it, or when nobody has anything else to do
      const unsigned long long m_wait = __ballot(alpha_wait && cur < 0);
      if (m_wait != 0ull && (__popcll(m_wait) >= kAlphaQuorum || __ballot((open || helper) && cur != kRayDone && !(alpha_wait && cur < 0)) == 0ull)) {
        if (alpha_wait && cur < 0) leaf_visit(std::true_type{});
      }
    }
#ifdef GLZ_SECTION_TIMES
    if (!PREFETCH) asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
#endif
    GLZ_SEC_STAMP(sec_leaf);
    // ---- merge: finished helpers hand their result to the owner of the ray ----
    if (SHARE) {
      // All helpers that are done leave together; only those that can have CHANGED their owner's result take a turn in the loop: a
      // helper that accepted a hit of its own (it starts from a copy of the donor's best, which the owner has) and, for closest-hit
      // rays, whose distance is still the smallest anyone has found for that ray (aux_t, kept by every lane of the tail at each
      // accepted hit: a result behind it cannot win, and whoever holds the smallest one either is the owner or will be here when it is
      // done).  A turn reads the helper's lane with v_readlane -- its index is wave uniform -- instead of through the LDS permute.
      // (tools/gpu_sections.py: a 1/8 share merged 71 helper results per wave and launch one after the other, 457 clocks each, 17 % of
      // the tracing time.)
      const bool done = helper && cur == kRayDone;
      bool cand = done && found_own;
      if (cand && !ANY && !any_lane) cand = __float_as_uint(best.t) == aux_t[ray];
      unsigned long long fin = __ballot(cand);
      while (fin != 0ull) {
#ifdef GLZ_SECTION_TIMES
        sec_merges += 1;
#endif
        const int h = __ffsll((long long)fin) - 1;   // wave uniform
        fin &= fin - 1ull;
        const int ow = __builtin_amdgcn_readlane((int)ray, h);
        const float bt = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(best.t), h));
        const float bu = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(best.u), h));
        const float bv = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(best.v), h));
        const uint32_t bl = (uint32_t)__builtin_amdgcn_readlane((int)best.leaf, h), bi = (uint32_t)__builtin_amdgcn_readlane((int)best_id, h);
        if (lane == ow) {
          const bool better = best.leaf == kNone ? true : (bt < best.t || (bt == best.t && bi < best_id));
          if (better) {
            best = HitRecord{bt, bu, bv, bl};
            best_id = bi;
          }
          if (any_lane) cur = kRayDone;   // occluded: the rest of the owner's stack does not matter
        }
      }
      if (done) {
        helper = false;
        atomicSub(&aux_out[ray], 1);
      }
    }
    GLZ_SEC_STAMP(sec_merge);
    // ---- retire ----
    // (Storing finished rays only when they make up a refill together with the idle lanes -- a fifth as many executions of the sink's code,
    // with a quarter of the wave in it instead of a lane or two: k_trace 0.483 against 0.483 ms, a 1/8 share 0.1312 against 0.1302.)
    if (open && cur == kRayDone && (!SHARE || aux_out[lane] == 0)) {
      if (COUNT) tally.hits += best.leaf != kNone;
      sink.store(ray, best);
      open = false;
    }
  }
  if (ROTATE) __builtin_amdgcn_s_setprio(0);
#ifdef GLZ_SECTION_TIMES
  {
    GLZ_SEC_STAMP(sec_tail);
    const uint32_t gw = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    if (lane == 0 && gw < 8192u) {
      unsigned long long* g = g_sections + 16 * gw;
      g[0] += sec_refill; g[1] += sec_share; g[2] += sec_node; g[3] += sec_ctl; g[4] += sec_leaf; g[5] += sec_tail;
      g[6] += sec_rounds; g[7] += sec_iters; g[8] += sec_leaves; g[9] += sec_takes; g[10] += 1; g[11] += sec_merges; g[12] += sec_merge; g[13] += sec_f0; g[14] += sec_f1; g[15] += sec_f2;
    }
  }
#endif
#ifdef GLZ_WAVE_TIMES
  if (!ANY && lane == 0 && wave < 8192u) {
    unsigned int* o = g_wave_stats + 8 * wave;
    o[0] = wt_rounds; o[1] = wt_node_iters; o[2] = wt_node_lanes; o[3] = wt_leaf_iters; o[4] = wt_leaf_lanes; o[5] = wt_helper_rounds; o[6] = wt_wait_rounds;
  }
#endif
}

__device__ __forceinline__ void flush_counters(TraceCounters* c, bool shadow, TraceTally t) {
  // wave-level reduction first, one atomic per wave and counter (Guideline 12)
  for (int off = 32; off > 0; off >>= 1) {
    t.rays += __shfl_down(t.rays, off);
    t.nodes += __shfl_down(t.nodes, off);
    t.tris += __shfl_down(t.tris, off);
    t.hits += __shfl_down(t.hits, off);
    t.fresh += __shfl_down(t.fresh, off);
  }
  if ((threadIdx.x & 63) == 0) {
    unsigned long long* ph = shadow ? c->phase + 6 : c->phase;
    atomicAdd(&ph[0], t.node_iters); atomicAdd(&ph[1], t.node_lanes); atomicAdd(&ph[2], t.leaf_iters); atomicAdd(&ph[3], t.leaf_lanes);
    atomicAdd(&ph[4], t.refill_iters); atomicAdd(&ph[5], t.refill_lanes);
  }
  if ((threadIdx.x & 63) == 0) {
    if (shadow) {
      atomicAdd(&c->shadow_rays, t.rays); atomicAdd(&c->shadow_nodes, t.nodes); atomicAdd(&c->shadow_tris, t.tris);
    } else {
      atomicAdd(&c->closest_rays, t.rays); atomicAdd(&c->closest_nodes, t.nodes); atomicAdd(&c->closest_tris, t.tris);
      atomicAdd(&c->hits, t.hits);
      atomicAdd(&c->fresh, t.fresh);
    }
  }
}

// a counting kernel's per-thread texture / light tallies (DeviceScene::tex_counter) -> the launch's counters: one atomic per wave and
// tally; every lane of the wave must get here
__device__ __forceinline__ void flush_tex_tallies(unsigned long long* dst, const unsigned long long* t) {
  unsigned long long a = t[0], b = t[1], c = t[2], d = t[3];
  for (int off = 32; off > 0; off >>= 1) {
    a += __shfl_down(a, off); b += __shfl_down(b, off); c += __shfl_down(c, off); d += __shfl_down(d, off);
  }
  if ((threadIdx.x & 63) == 0) {
    atomicAdd(dst, a); atomicAdd(dst + 1, b); atomicAdd(dst + 2, c); atomicAdd(dst + 3, d);
  }
}

// persistent launch geometry: every wave of the grid is one independent tracer
// (XCD-aware numbering -- the blocks with b % 8 == x, which share an L2, taking one contiguous run of groups / pixels each,
// cdna_hip_programming.md T1 -- measured slower for both kernels: k_trace 0.588 -> 0.621 ms, k_shade 0.348 -> 0.357 ms, a 1/8
// share 0.162 -> 0.188 ms.  Neighbouring regions differ in cost; dealing them round-robin over the XCDs balances that, and
// the L2s' hit rates are not what bounds either kernel.)
__device__ __forceinline__ uint32_t wave_index() { return blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6); }
__device__ __forceinline__ uint32_t wave_count() { return gridDim.x * (kBlock / 64); }

// copies the scene's top-of-tree table (types.h kBvhTopNodes) into the block's LDS; ends with a block barrier
__device__ __forceinline__ void stage_top(const DeviceScene& S, uint4* s_top) {
  const uint4* src = reinterpret_cast<const uint4*>(S.bvh_top);
  if (threadIdx.x < kBvhTopNodes * 4) s_top[threadIdx.x] = src[threadIdx.x];
  __syncthreads();
}

#ifdef GLZ_WAVE_TIMES   // tuning builds only (tools/build_variant.sh, tools/gpu_wave_times.py): when each wave of the last k_trace with closest-hit rays started, finished those and ended
#define GLZ_WAVE_STAMP(k) do { if (A.do_closest && (threadIdx.x & 63) == 0 && wave_index() < 8192u) g_wave_times[3 * wave_index() + (k)] = wall_clock64(); } while (0)
#else
#define GLZ_WAVE_STAMP(k) do { } while (0)
#endif
}  // namespace glz
