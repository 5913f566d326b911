// Vertex normals recomputed from deformed positions (glz_renderer_add_normals, glz_host_vertex_normals; include/glaze_abi.h holds the
// specification, "THE NORMAL RULE"): a face's vector and a vertex's normal in the ONE form both the host reference (normals_host.cpp; g++)
// and the device kernels (kernels_normals.hip; hipcc) compile: the same operations in the same order, -ffp-contract=off on both sides, so
// the two agree bit for bit.  float32, only + - *, one sqrtf and one 1.0f / x, both correctly rounded on either side.
//
// THE LAYOUT both sides read (NormalLayout; pack_normals makes it once, on the host).  The FACES of a set are the scene's triangles with
// at least one corner in the set's range, in (mesh, triangle) order: three global vertex indices a face.  A vertex's ROW is the ascending
// list of the faces that touch its group -- every member of a group carries the group's whole row, so the sum's order is the row's order
// and nothing else decides it.  The rows are stored as morph.h stores its own: sliced ELLPACK whose slice is one wavefront.  The set's
// vertices are taken in groups of kNormalSlice = 64 from its own first vertex; vertex v has counts[v] faces, slice s has the width W_s of
// its longest row and starts at uint32 number slices[s].x of `rows`; step k of a slice is 64 consecutive uint32, one a lane -- what a wave
// reads in one access is 256 consecutive bytes.  Slots past a row's count are padding: zero, which a kernel may read as
// face 0 and never adds.
#pragma once
#include <math.h>

#include <string>
#include <vector>

#include "denoise.h"

namespace glz {
namespace post {

constexpr uint32_t kNormalSlice = 64;   // vertices a slice: one wavefront

// The face vector of corner positions p0, p1, p2 (their .w is not looked at): the cross product of the two edges from p0, whose length --
// twice the face's area -- is the face's weight in every sum it enters.  .w is +0.
GLZ_POST_FN float4 face_vector(float4 p0, float4 p1, float4 p2) {
  const float ax = p1.x - p0.x, ay = p1.y - p0.y, az = p1.z - p0.z;
  const float bx = p2.x - p0.x, by = p2.y - p0.y, bz = p2.z - p0.z;
  return make_float4(ay * bz - az * by, az * bx - ax * bz, ax * by - ay * bx, 0.0f);
}

// One vertex's normal.  lane_row: the uint32 of the vertex's slice at its own lane (rows + slices[s].x + lane); steps: the trip count of
// the loop, at least `count` -- the host passes the row's count itself, a kernel its slice's width, which is the same for all lanes of the
// wave; count: the row's length, past which nothing is added; faces: one float4 a face of the set, in whichever memory
// Faces names.  S starts from +0 and takes the faces in the row's order; the result has the form of normalize3 (device/math.h) where the
// squared length is positive and finite, and is S itself elsewhere (zeros, NaN and overflow go through as the arithmetic makes them).
//
// The walk goes kNormalChunk steps at a time: first the chunk's face numbers, then the face vectors they name, then the additions, in the
// row's order.  That changes no bit -- the additions are the same and in the same order -- and lets a kernel have a chunk's loads in
// flight together where a step-by-step walk waits for two dependent loads a step.  Steps of the chunk past `steps` read step `steps - 1` again (an index
// that is clamped, not a branch: a branch a load keeps the loads apart) and add nothing; steps from `count` up to `steps` read the
// slice's padding, which is zero, so face 0, and add nothing: the host, whose steps are its count, never reads padding at all.
constexpr uint32_t kNormalChunk = 8;
template <class Row, class Faces>
GLZ_POST_FN float4 vertex_normal(Row lane_row, uint32_t steps, uint32_t count, Faces faces) {
  float sx = 0.0f, sy = 0.0f, sz = 0.0f;
  for (uint32_t k = 0; k < steps; k += kNormalChunk) {
    uint32_t face[kNormalChunk];
    float4 f[kNormalChunk];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (uint32_t u = 0; u < kNormalChunk; ++u) face[u] = lane_row[(size_t)(k + u < steps ? k + u : steps - 1) * kNormalSlice];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (uint32_t u = 0; u < kNormalChunk; ++u) f[u] = faces[face[u]];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (uint32_t u = 0; u < kNormalChunk; ++u) {
      if (k + u < count) {
        sx = sx + f[u].x;
        sy = sy + f[u].y;
        sz = sz + f[u].z;
      }
    }
  }
  const float d = (sx * sx + sy * sy) + sz * sz;
  if (d > 0.0f && d < INFINITY) {
    const float inv = 1.0f / sqrtf(d);
    return make_float4(sx * inv, sy * inv, sz * inv, 0.0f);
  }
  return make_float4(sx, sy, sz, 0.0f);
}

struct NormalLayout {
  uint32_t first = 0, n_vertices = 0;   // the set's range of the scene's vertices
  uint32_t n_faces = 0;
  uint32_t reach_lo = 0, reach_hi = 0;  // the lowest and the highest vertex index of any corner of the faces (n_faces > 0)
  uint64_t n_entries = 0;               // row entries that are not padding: the sum of counts
  std::vector<uint32_t> faces;          // 3 a face: global vertex indices; never empty (three zeros when there is no face)
  std::vector<uint32_t> counts;         // one a vertex
  std::vector<uint2> slices;            // one a slice: (first uint32 of the slice in `rows`, W_s)
  std::vector<uint32_t> rows;           // sum over the slices of W_s * kNormalSlice; never empty (one zero when no vertex has a face)
};

// The checks of a normal set (glz_renderer_add_normals lists them; overlap with other sets is the scene's to check) and the layout; false
// with `why` set, `out` unspecified.  indices / meshes: the scene's, every mesh's index range inside n_indices and every index below
// n_scene_vertices (creation has checked; checked again here, since glz_host_vertex_normals takes raw arrays).
bool pack_normals(const uint32_t* indices, uint64_t n_indices, const glz_mesh* meshes, uint64_t n_meshes, uint64_t n_scene_vertices, uint32_t first,
                  uint32_t n_vertices, const uint32_t* groups, NormalLayout& out, std::string& why);

// the reference on host arrays (normals_host.cpp): `vertices` is the scene's whole vertex array, read at every corner of the layout's
// faces; out: the layout's n_vertices vertices, the range's own with their normal words replaced where the row is not empty; out may be
// vertices + first itself (the face vectors are all taken before the first vertex is written)
void host_vertex_normals(const glz_vertex* vertices, const NormalLayout& layout, glz_vertex* out);

// the label of vertex i is the lowest j <= i of the range whose three position words and three normal words are bit-equal to i's
void host_weld_groups(const glz_vertex* vertices, uint32_t n, uint32_t* groups_out);

}  // namespace post
}  // namespace glz
