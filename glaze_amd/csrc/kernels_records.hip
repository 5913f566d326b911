// Kernels the scene runs on its own, outside any hierarchy build: per-triangle derivatives, the per-leaf shading and alpha-test
// records, and the top-of-tree table of the tracers' LDS staging.
#include <hip/hip_runtime.h>

#include "build_common.h"
#include "device/math.h"
#include "kernels.h"

namespace glz {
using namespace dev;

// ---------------------------------------------------------------------------------------------
// generate_derivatives.comp:23-64 -- one thread per object-space triangle, 48 bytes out
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_tri_derivatives(const float4* __restrict__ vertices, const uint32_t* __restrict__ indices,
                                                         uint32_t n_tris, float4* __restrict__ out) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_tris) return;
  const uint32_t i0 = indices[3 * t], i1 = indices[3 * t + 1], i2 = indices[3 * t + 2];
  const float4 a0 = vertices[2 * i0], a1 = vertices[2 * i0 + 1];
  const float4 b0 = vertices[2 * i1], b1 = vertices[2 * i1 + 1];
  const float4 c0 = vertices[2 * i2], c1 = vertices[2 * i2 + 1];
  const vec3 p0 = mk3(a0.x, a0.y, a0.z), p1 = mk3(b0.x, b0.y, b0.z), p2 = mk3(c0.x, c0.y, c0.z);
  // texcoords are the last two floats of the packed vertex (raytrace_commons.glsl:28-31)
  const float duv02x = a1.z - c1.z, duv02y = a1.w - c1.w;
  const float duv12x = b1.z - c1.z, duv12y = b1.w - c1.w;
  const float det = duv02x * duv12y - duv02y * duv12x;
  const vec3 n = normalize3(cross3(p1 - p0, p2 - p0));
  vec3 dpdu, dpdv;
  if (det == 0.0f) {
    if (fabsf(n.x) > fabsf(n.y)) dpdu = mk3(-n.z, 0.0f, n.x) / sqrtf(n.x * n.x + n.z * n.z);
    else dpdu = mk3(0.0f, n.z, -n.y) / sqrtf(n.y * n.y + n.z * n.z);
    dpdv = cross3(n, dpdu);
  } else {
    const vec3 dp02 = p0 - p2, dp12 = p1 - p2;
    const float invdet = 1.0f / det;
    dpdu = (duv12y * dp02 - duv02y * dp12) * invdet;
    dpdv = ((-duv12x) * dp02 + duv02x * dp12) * invdet;
  }
  out[3 * t] = make_float4(n.x, n.y, n.z, 0.0f);
  out[3 * t + 1] = make_float4(dpdu.x, dpdu.y, dpdu.z, 0.0f);
  out[3 * t + 2] = make_float4(dpdv.x, dpdv.y, dpdv.z, 0.0f);
}

// Per-leaf shading records: everything raytrace_hit.rchit reads for a hit (3 packed vertices, the triangle's
// derivatives, material and transform ids) gathered into one contiguous 128-byte record so that k_shade fetches it
// with 8 dwordx4 loads instead of walking leaf -> instance -> indices -> vertices -> derivatives (14 scattered loads,
// three levels of dependent latency).
__global__ void __launch_bounds__(256) k_shade_records(uint32_t n, const BvhTri* __restrict__ tris, const RTInstance* __restrict__ instances,
                                                       const uint32_t* __restrict__ indices, const float4* __restrict__ vertices,
                                                       const float4* __restrict__ derivatives, const uint32_t* __restrict__ xf_identity,
                                                       float4* __restrict__ out) {
  const uint32_t leaf = blockIdx.x * blockDim.x + threadIdx.x;
  if (leaf >= n) return;
  const BvhTri t = tris[leaf];
  const RTInstance in = instances[t.instance];
  const uint32_t tri_id = in.index_offset / 3u + (t.prim_flags & kTriPrimMask);
  float4* r = out + 8 * (size_t)leaf;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const uint32_t v = indices[3u * tri_id + k];
    r[2 * k] = vertices[2u * v];
    r[2 * k + 1] = vertices[2u * v + 1u];
  }
  const float4 dn = derivatives[3u * tri_id], du = derivatives[3u * tri_id + 1u];
  r[6] = make_float4(dn.x, dn.y, dn.z, __uint_as_float(in.material_id));
  r[7] = make_float4(du.x, du.y, du.z, __uint_as_float(in.transform_id | (xf_identity[in.transform_id] ? 0x80000000u : 0u)));
}

// The alpha test's inputs per triangle slot (types.h DeviceScene::alpha_recs): the three texture coordinates out of the shading record
// and the descriptor of the material's opacity map, side by side.  A slot whose material has no opacity map gets a record nobody reads.
__global__ void __launch_bounds__(256) k_alpha_records(uint32_t n, const float4* __restrict__ shade_tris, const RTMaterial* __restrict__ materials,
                                                       const TexDesc* __restrict__ tex_desc, float4* __restrict__ out) {
  const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
  if (slot >= n) return;
  const float4* rec = shade_tris + 8u * (size_t)slot;
  const float4 a = rec[1], b = rec[3], c = rec[5];
  const uint32_t opacity = materials[__float_as_uint(rec[6].w)].opacity;
  const TexDesc t = tex_desc[opacity];
  float4* r = out + 3u * (size_t)slot;
  r[0] = make_float4(a.z, a.w, b.z, b.w);
  r[1] = make_float4(c.z, c.w, __uint_as_float(t.offset), __uint_as_float(t.width));
  r[2] = make_float4(__uint_as_float(t.height), __uint_as_float(t.format), 0.0f, 0.0f);
}

// Top-of-tree table (types.h kBvhTopNodes): breadth-first from the root, one thread -- 21 dependent 64-byte reads, once per
// scene.  An inner child gets the next free slot and its link in the table becomes kBvhTopFlag | slot; leaves, empty
// slots and inner children beyond the table keep their links.  Unused slots stay zero (never referenced).
__global__ void k_top_table(const BvhNode4* __restrict__ nodes, uint32_t n_nodes, BvhNode4* __restrict__ top) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  for (int s = 0; s < kBvhTopNodes; ++s)
    for (int k = 0; k < 16; ++k) top[s].w[k] = 0u;
  if (n_nodes == 0) return;
  int source[kBvhTopNodes];
  int used = 1;
  source[0] = 0;
  for (int s = 0; s < used; ++s) {
    BvhNode4 nd = nodes[source[s]];
    for (int k = 0; k < 4; ++k) {
      const int link = (int)nd.w[12 + k];
      if (link >= 0 && link != kBvhEmptyChild && (uint32_t)link < n_nodes && used < kBvhTopNodes) {
        source[used] = link;
        nd.w[12 + k] = (uint32_t)(kBvhTopFlag | used);
        ++used;
      }
    }
    top[s] = nd;
  }
}

hipError_t launch_derivatives(hipStream_t st, const float4* vertices, const uint32_t* indices, uint32_t n_tris, float4* out) {
  if (n_tris == 0) return hipSuccess;
  // the reference dispatches (triangles/256)+1 groups of 256 (scene.rs:2162)
  return launch(k_tri_derivatives, dim3(n_tris / 256 + 1), dim3(256), st, vertices, indices, n_tris, out);
}

hipError_t launch_top_table(hipStream_t st, const BvhNode4* nodes, uint32_t n_nodes, BvhNode4* top) {
  return launch(k_top_table, dim3(1), dim3(64), st, nodes, n_nodes, top);
}

hipError_t launch_shade_records(hipStream_t st, uint32_t n, const BvhTri* tris, const RTInstance* instances, const uint32_t* indices,
                                const float4* vertices, const float4* derivatives, const uint32_t* xf_identity, float4* out) {
  if (n == 0) return hipSuccess;
  return launch(k_shade_records, dim3((n + 255) / 256), dim3(256), st, n, tris, instances, indices, vertices, derivatives, xf_identity, out);
}

hipError_t launch_alpha_records(hipStream_t st, uint32_t n, const float4* shade_tris, const RTMaterial* materials, const TexDesc* tex_desc, float4* out) {
  if (n == 0) return hipSuccess;
  return launch(k_alpha_records, dim3((n + 255) / 256), dim3(256), st, n, shade_tris, materials, tex_desc, out);
}

}  // namespace glz
