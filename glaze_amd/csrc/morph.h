// Morph targets / blend shapes (glz_renderer_add_morph, glz_renderer_animate, glz_host_morph; include/glaze_abi.h holds the specification,
// "THE MORPH RULE"): one vertex under the targets that touch it, in the ONE form both the host reference (morph_host.cpp; g++) and the
// device kernels (kernels_morph.hip; hipcc) compile: the same operations in the same order, -ffp-contract=off on both sides, so the two
// agree bit for bit.  Only + and *, float32.
//
// THE LAYOUT both sides read (MorphLayout; pack_morph makes it once, on the host): sliced ELLPACK whose slice is one wavefront.  The
// morph's vertices are taken in groups of kMorphSlice = 64 from its own first vertex; vertex v has counts[v] entries (its row), slice s
// has the width W_s of its longest row and starts at float4 number slices[s].x of `entries`.  The entries of a slice are stored step-major
// in two planes a step: step k holds 64 float4 (d_position.xyz, the target's index as the bits of .w), one a lane, then 64 float4
// (d_normal.xyz, 0) -- so what the 64 lanes of a wave read in one access is one whole kilobyte of consecutive float4.  A row's entries are
// in ascending target order, which is the order the rule adds them in.  Slots past a row's count are padding: zero, never read.
#pragma once
#include <string.h>

#include <string>
#include <vector>

#include "denoise.h"

namespace glz {
namespace post {

constexpr uint32_t kMorphSlice = 64;                   // vertices a slice: one wavefront
constexpr uint32_t kMorphStepStride = 2 * kMorphSlice;  // float4 a step of a slice: the position plane, then the normal plane
constexpr uint32_t kMorphMaxTargets = 65536;

GLZ_POST_FN uint32_t word_of(float f) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __float_as_uint(f);
#else
  uint32_t u;
  memcpy(&u, &f, sizeof u);
  return u;
#endif
}

// One vertex: v0 = (p.xyz, n.x), v1 = (n.yz, t.uv) as the vertex buffer stores it, in and out.  lane_entries: the float4 of the vertex's
// slice at its own lane (entries + slices[s].x + lane); steps: the trip count of the loop, at least `count` -- the host passes the row's
// count itself, a kernel its slice's width, which is the same for all lanes of the wave; count: the vertex's row length, past which
// nothing is read and nothing is computed (the rule adds no term); weights: one float a target, in whichever memory Weights names.
template <class Entries, class Weights>
GLZ_POST_FN void morph_vertex(Entries lane_entries, uint32_t steps, uint32_t count, Weights weights, float4& v0, float4& v1) {
  for (uint32_t k = 0; k < steps; ++k) {
    if (k < count) {
      const float4 dp = lane_entries[(size_t)k * kMorphStepStride], dn = lane_entries[(size_t)k * kMorphStepStride + kMorphSlice];
      const float w = weights[word_of(dp.w)];
      v0 = make_float4(v0.x + w * dp.x, v0.y + w * dp.y, v0.z + w * dp.z, v0.w + w * dn.x);
      v1 = make_float4(v1.x + w * dn.y, v1.y + w * dn.z, v1.z, v1.w);
    }
  }
}

struct MorphLayout {
  uint32_t n_vertices = 0, n_targets = 0;
  uint64_t n_entries = 0;          // entries that are not padding: the sum of counts
  std::vector<uint32_t> counts;    // one a vertex
  std::vector<uint2> slices;       // one a slice: (first float4 of the slice in `entries`, W_s)
  std::vector<float4> entries;     // sum over the slices of W_s * kMorphStepStride; never empty (one zero float4 when no target has an entry)
};

// The checks of a morph's targets (glz_renderer_add_morph lists them) and the layout; false with `why` set, `out` unspecified.
bool pack_morph(uint32_t n_vertices, const glz_morph_target* targets, uint32_t n_targets, MorphLayout& out, std::string& why);

// the reference on host arrays (morph_host.cpp): base[v] under the layout's rows and `weights` (one a target); out may be `base` itself
void host_morph(const glz_vertex* base, const MorphLayout& layout, const float* weights, glz_vertex* out);

}  // namespace post
}  // namespace glz
