// glz_host_vertex_normals, glz_host_weld_groups and the layout packer: the normal rule of normals.h on the host cores, no device -- the
// reference k_face_vectors and k_vertex_normals are compared with bit for bit -- and the making of the face list and the per-vertex rows
// both sides read.
#include "normals.h"

#include <stddef.h>
#include <string.h>

#include <algorithm>
#include <array>
#include <numeric>

namespace glz {
namespace post {

bool pack_normals(const uint32_t* indices, uint64_t n_indices, const glz_mesh* meshes, uint64_t n_meshes, uint64_t n_scene_vertices, uint32_t first,
                  uint32_t n_vertices, const uint32_t* groups, NormalLayout& out, std::string& why) {
  auto refuse = [&](const char* w) {
    why = w;
    return false;
  };
  if (n_vertices == 0 || (uint64_t)first + n_vertices > n_scene_vertices) return refuse("no vertices, or a range past the vertex count");
  if ((n_indices && !indices) || (n_meshes && !meshes)) return refuse("the indices or the meshes are null");
  if (groups)
    for (uint32_t v = 0; v < n_vertices; ++v)
      if (groups[v] >= n_vertices) return refuse("a group label is not below n_vertices");
  for (uint64_t m = 0; m < n_meshes; ++m)
    if ((uint64_t)meshes[m].index_offset + meshes[m].index_count > n_indices) return refuse("a mesh's index range is past the index count");
  out = NormalLayout{};
  out.first = first;
  out.n_vertices = n_vertices;
  const uint64_t last = (uint64_t)first + n_vertices;
  auto in_range = [&](uint32_t c) { return c >= first && c < last; };
  auto group_of = [&](uint32_t c) { return groups ? groups[c - first] : c - first; };
  // Two walks over the triangles in (mesh, triangle) order, the same each time: the first numbers the faces and counts each group's, the
  // second fills the groups' lists.  seen[g] is the last face put to group g: a face enters a group once, however many of its corners
  // (or of the group's members) meet there, and the lists come out ascending because the face numbers only grow.
  constexpr uint32_t kNone = 0xFFFFFFFFu;
  std::vector<uint32_t> seen(n_vertices, kNone);
  std::vector<uint64_t> start((size_t)n_vertices + 1, 0);
  uint32_t lo = kNone, hi = 0;
  for (uint64_t m = 0; m < n_meshes; ++m) {
    const uint32_t* tri = indices + meshes[m].index_offset;
    for (uint32_t k = 0; k < meshes[m].index_count / 3; ++k, tri += 3) {
      for (int c = 0; c < 3; ++c)
        if (tri[c] >= n_scene_vertices) return refuse("an index is not below the vertex count");
      if (!in_range(tri[0]) && !in_range(tri[1]) && !in_range(tri[2])) continue;
      if (out.faces.size() / 3 >= kNone) return refuse("more faces than a row can name");
      const uint32_t f = (uint32_t)(out.faces.size() / 3);
      for (int c = 0; c < 3; ++c) {
        out.faces.push_back(tri[c]);
        lo = std::min(lo, tri[c]);
        hi = std::max(hi, tri[c]);
        if (!in_range(tri[c])) continue;
        const uint32_t g = group_of(tri[c]);
        if (seen[g] != f) {
          seen[g] = f;
          ++start[(size_t)g + 1];
        }
      }
    }
  }
  out.n_faces = (uint32_t)(out.faces.size() / 3);
  out.reach_lo = out.n_faces ? lo : 0;
  out.reach_hi = hi;
  for (size_t g = 0; g < n_vertices; ++g) start[g + 1] += start[g];
  std::vector<uint32_t> lists((size_t)start[n_vertices]);
  std::vector<uint64_t> fill(start.begin(), start.end() - 1);
  std::fill(seen.begin(), seen.end(), kNone);
  for (uint32_t f = 0; f < out.n_faces; ++f)
    for (int c = 0; c < 3; ++c) {
      const uint32_t corner = out.faces[3 * (size_t)f + c];
      if (!in_range(corner)) continue;
      const uint32_t g = group_of(corner);
      if (seen[g] != f) {
        seen[g] = f;
        lists[(size_t)fill[g]++] = f;
      }
    }
  if (out.faces.empty()) out.faces.assign(3, 0u);
  // every member of a group carries the group's row
  out.counts.resize(n_vertices);
  for (uint32_t v = 0; v < n_vertices; ++v) {
    const uint32_t g = groups ? groups[v] : v;
    const uint64_t count = start[(size_t)g + 1] - start[g];
    out.counts[v] = (uint32_t)count;
    out.n_entries += count;
  }
  const size_t n_slices = ((size_t)n_vertices + kNormalSlice - 1) / kNormalSlice;
  out.slices.resize(n_slices);
  uint64_t total = 0;
  for (size_t s = 0; s < n_slices; ++s) {
    uint32_t width = 0;
    for (size_t v = s * kNormalSlice; v < std::min<size_t>((s + 1) * kNormalSlice, n_vertices); ++v) width = std::max(width, out.counts[v]);
    if (total > 0xFFFFFFFFull) return refuse("the layout is too large (a slice would start past 2^32 entries)");
    out.slices[s] = make_uint2((uint32_t)total, width);
    total += (uint64_t)width * kNormalSlice;
  }
  out.rows.assign((size_t)std::max<uint64_t>(total, 1), 0u);
  for (uint32_t v = 0; v < n_vertices; ++v) {
    const uint32_t g = groups ? groups[v] : v;
    uint32_t* lane_row = out.rows.data() + out.slices[v / kNormalSlice].x + v % kNormalSlice;
    for (uint32_t k = 0; k < out.counts[v]; ++k) lane_row[(size_t)k * kNormalSlice] = lists[(size_t)start[g] + k];
  }
  return true;
}

void host_vertex_normals(const glz_vertex* vertices, const NormalLayout& layout, glz_vertex* out) {
  std::vector<float4> face_vectors(std::max<size_t>(layout.n_faces, 1), make_float4(0.0f, 0.0f, 0.0f, 0.0f));
  auto position = [&](uint32_t i) { return make_float4(vertices[i].vv[0], vertices[i].vv[1], vertices[i].vv[2], 0.0f); };
  for (size_t f = 0; f < layout.n_faces; ++f)
    face_vectors[f] = face_vector(position(layout.faces[3 * f]), position(layout.faces[3 * f + 1]), position(layout.faces[3 * f + 2]));
  for (size_t i = 0; i < layout.n_vertices; ++i) {
    glz_vertex v = vertices[layout.first + i];
    if (layout.counts[i] != 0) {
      const uint32_t* lane_row = layout.rows.data() + layout.slices[i / kNormalSlice].x + i % kNormalSlice;
      const float4 n = vertex_normal(lane_row, layout.counts[i], layout.counts[i], face_vectors.data());
      v.vn[0] = n.x;
      v.vn[1] = n.y;
      v.vn[2] = n.z;
    }
    out[i] = v;
  }
}

void host_weld_groups(const glz_vertex* vertices, uint32_t n, uint32_t* groups_out) {
  using Key = std::array<uint32_t, 6>;   // the position's and the normal's words as they are: -0 is not +0, a NaN equals its own bits
  auto key = [&](uint32_t i) {
    Key k;
    memcpy(k.data(), vertices[i].vv, sizeof(uint32_t) * 6);
    return k;
  };
  static_assert(offsetof(glz_vertex, vn) == 3 * sizeof(float), "position and normal are six consecutive words");
  std::vector<uint32_t> order(n);
  std::iota(order.begin(), order.end(), 0u);
  std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
    const Key ka = key(a), kb = key(b);
    return ka != kb ? ka < kb : a < b;
  });
  for (uint32_t at = 0; at < n;) {
    const uint32_t label = order[at];   // the lowest index of its run
    const Key k = key(label);
    for (; at < n && key(order[at]) == k; ++at) groups_out[order[at]] = label;
  }
}

}  // namespace post
}  // namespace glz
