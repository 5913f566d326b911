// glz_host_morph and the layout packer: the morph rule of morph.h on the host cores, no device -- the reference k_morph and k_morph_skin are
// compared with bit for bit -- and the transposition of per-target lists into the sliced layout both sides read.
#include "morph.h"

#include <algorithm>

namespace glz {
namespace post {

bool pack_morph(uint32_t n_vertices, const glz_morph_target* targets, uint32_t n_targets, MorphLayout& out, std::string& why) {
  auto refuse = [&](const char* w) {
    why = w;
    return false;
  };
  if (!targets) return refuse("the targets are null");
  if (n_targets == 0 || n_targets > kMorphMaxTargets) return refuse("n_targets must be 1 .. 65536");
  out = MorphLayout{};
  out.n_vertices = n_vertices;
  out.n_targets = n_targets;
  out.counts.assign(n_vertices, 0u);
  for (uint32_t t = 0; t < n_targets; ++t) {
    const glz_morph_target& g = targets[t];
    if (g.n == 0) continue;
    if (!g.d_position || !g.d_normal) return refuse("a target with entries has null deltas");
    if (!g.vertices) {
      if (g.n != n_vertices) return refuse("a dense target must have one entry a vertex");
      for (uint32_t v = 0; v < n_vertices; ++v) ++out.counts[v];
      continue;
    }
    for (uint32_t e = 0; e < g.n; ++e) {
      if (g.vertices[e] >= n_vertices) return refuse("a target's entry names a vertex past n_vertices");
      if (e > 0 && g.vertices[e] <= g.vertices[e - 1]) return refuse("a target's vertex indices are not strictly ascending");
      ++out.counts[g.vertices[e]];
    }
  }
  const size_t n_slices = ((size_t)n_vertices + kMorphSlice - 1) / kMorphSlice;
  out.slices.resize(n_slices);
  uint64_t total = 0;
  for (size_t s = 0; s < n_slices; ++s) {
    uint32_t width = 0;
    for (size_t v = s * kMorphSlice; v < std::min<size_t>((s + 1) * kMorphSlice, n_vertices); ++v) {
      width = std::max(width, out.counts[v]);
      out.n_entries += out.counts[v];
    }
    if (total > 0xFFFFFFFFull) return refuse("the layout is too large (a slice would start past 2^32 entries)");
    out.slices[s] = make_uint2((uint32_t)total, width);
    total += (uint64_t)width * kMorphStepStride;
  }
  out.entries.assign((size_t)std::max<uint64_t>(total, 1), make_float4(0.0f, 0.0f, 0.0f, 0.0f));
  std::vector<uint32_t> filled(n_vertices, 0u);
  for (uint32_t t = 0; t < n_targets; ++t) {   // ascending targets: a row's entries come out in the rule's order
    const glz_morph_target& g = targets[t];
    float id;
    memcpy(&id, &t, sizeof id);
    for (uint32_t e = 0; e < g.n; ++e) {
      const uint32_t v = g.vertices ? g.vertices[e] : e;
      const size_t at = (size_t)out.slices[v / kMorphSlice].x + (size_t)filled[v]++ * kMorphStepStride + v % kMorphSlice;
      out.entries[at] = make_float4(g.d_position[3 * (size_t)e], g.d_position[3 * (size_t)e + 1], g.d_position[3 * (size_t)e + 2], id);
      out.entries[at + kMorphSlice] = make_float4(g.d_normal[3 * (size_t)e], g.d_normal[3 * (size_t)e + 1], g.d_normal[3 * (size_t)e + 2], 0.0f);
    }
  }
  return true;
}

void host_morph(const glz_vertex* base, const MorphLayout& layout, const float* weights, glz_vertex* out) {
  for (size_t i = 0; i < layout.n_vertices; ++i) {
    const glz_vertex v = base[i];
    float4 v0 = make_float4(v.vv[0], v.vv[1], v.vv[2], v.vn[0]), v1 = make_float4(v.vn[1], v.vn[2], v.vt[0], v.vt[1]);
    const float4* lane_entries = layout.entries.data() + layout.slices[i / kMorphSlice].x + i % kMorphSlice;
    morph_vertex(lane_entries, layout.counts[i], layout.counts[i], weights, v0, v1);
    out[i] = glz_vertex{{v0.x, v0.y, v0.z}, {v0.w, v1.x, v1.y}, {v1.z, v1.w}};
  }
}

}  // namespace post
}  // namespace glz
