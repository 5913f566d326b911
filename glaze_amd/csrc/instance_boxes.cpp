// The host side of the instance boxes (instance_boxes.h).
#include "instance_boxes.h"

#include <algorithm>
#include <cmath>

namespace glz {

const glz_mesh* mesh_by_id(const SceneData& d, uint32_t id) {
  const glz_mesh* found = nullptr;
  for (const glz_mesh& m : d.meshes)
    if (m.id == id) found = &m;
  return found;
}

// load_raytrace_instances_to_gpu (scene.rs:1784-1818): dangling instances dropped
std::vector<RTInstance> rt_instances(const SceneData& d) {
  std::vector<RTInstance> out;
  for (const glz_mesh_instance& in : d.instances) {
    const glz_mesh* found = mesh_by_id(d, in.mesh_id);
    if (!found) continue;
    out.push_back(RTInstance{found->index_offset, found->index_count, found->material, in.transform_id});
  }
  return out;
}

std::vector<std::pair<uint32_t, uint32_t>> unique_meshes(const std::vector<RTInstance>& instances, std::vector<uint32_t>& mesh_of) {
  std::vector<std::pair<uint32_t, uint32_t>> ranges;
  mesh_of.resize(instances.size());
  for (size_t i = 0; i < instances.size(); ++i) {
    const std::pair<uint32_t, uint32_t> key(instances[i].index_offset, instances[i].index_count);
    const size_t m = std::find(ranges.begin(), ranges.end(), key) - ranges.begin();
    if (m == ranges.size()) ranges.push_back(key);
    mesh_of[i] = (uint32_t)m;
  }
  return ranges;
}

bool valid_geometry(const SceneData& d, size_t n_transforms, Error& err) {
  for (const glz_mesh& m : d.meshes)
    if ((uint64_t)m.index_offset + m.index_count > d.indices.size()) return err.fail(GLZ_E_INVALID_DATA, "mesh index range outside the index buffer");
  for (uint32_t i : d.indices)
    if (i >= d.vertices.size()) return err.fail(GLZ_E_INVALID_DATA, "vertex index out of range");
  for (const glz_mesh_instance& in : d.instances)
    if (in.transform_id >= n_transforms) return err.fail(GLZ_E_INVALID_DATA, "instance references a missing transform");
  return true;
}

// ---- instance boxes of the top level: world AABB of the mesh's VERTICES under the instance's transform, padded.  (The eight corners
// of the mesh's object box, which is what a top level normally takes, give a box up to sqrt(2) too wide per axis for a rotated
// instance -- a quarter more instance entries per ray in the column forest.  The vertices cost instances x vertices; past `budget`
// point transforms the remaining instances fall back to the corners.) ----
std::vector<std::vector<float>> mesh_points(const SceneData& d, const std::vector<std::pair<uint32_t, uint32_t>>& ranges) {
  std::vector<std::vector<float>> out(ranges.size());   // xyz of the vertices a mesh references, once each, in first-use order
  std::vector<uint8_t> seen(d.vertices.size(), 0);
  for (size_t mi = 0; mi < ranges.size(); ++mi) {
    const uint32_t off = ranges[mi].first, count = ranges[mi].second;
    std::vector<float>& pts = out[mi];
    for (uint32_t k = 0; k < count; ++k) {
      const uint32_t v = d.indices[off + k];
      if (seen[v]) continue;
      seen[v] = 1;
      pts.insert(pts.end(), d.vertices[v].vv, d.vertices[v].vv + 3);
    }
    for (uint32_t k = 0; k < count; ++k) seen[d.indices[off + k]] = 0;
  }
  return out;
}

std::vector<uint8_t> exact_box_instances(const std::vector<uint32_t>& mesh_of, const std::vector<uint64_t>& mesh_point_count, uint64_t budget) {
  std::vector<uint8_t> exact(mesh_of.size(), 0);
  uint64_t spent = 0;
  for (size_t i = 0; i < mesh_of.size(); ++i) {
    const uint64_t n = mesh_point_count[mesh_of[i]];
    if (n != 0 && spent + n <= budget) {
      spent += n;
      exact[i] = 1;
    }
  }
  return exact;
}

void host_instance_boxes(const std::vector<uint32_t>& mesh_of, const std::vector<uint32_t>& transform_of, const std::vector<InstanceBoxMesh>& meshes,
                         const std::vector<glz_transform>& transforms, uint64_t budget, std::vector<float4>& blo, std::vector<float4>& bhi) {
  const size_t ni = mesh_of.size();
  blo.assign(ni, float4{});
  bhi.assign(ni, float4{});
  std::vector<uint64_t> counts(meshes.size());
  for (size_t m = 0; m < meshes.size(); ++m) counts[m] = meshes[m].points.size() / 3;
  const std::vector<uint8_t> exact = exact_box_instances(mesh_of, counts, budget);
  for (size_t i = 0; i < ni; ++i) {
    const InstanceBoxMesh& m = meshes[mesh_of[i]];
    const float* M = transforms[transform_of[i]].m;
    double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
    auto take = [&](double x, double y, double z) {
      for (int k = 0; k < 3; ++k) {
        const double w = (double)M[k] * x + (double)M[4 + k] * y + (double)M[8 + k] * z + (double)M[12 + k];
        lo[k] = std::min(lo[k], w);
        hi[k] = std::max(hi[k], w);
      }
    };
    const std::vector<float>& pts = m.points;
    if (exact[i]) {
      for (size_t k = 0; k + 2 < pts.size(); k += 3) take(pts[k], pts[k + 1], pts[k + 2]);
    } else {
      for (int c = 0; c < 8; ++c) take((c & 1) ? m.hi[0] : m.lo[0], (c & 2) ? m.hi[1] : m.lo[1], (c & 4) ? m.hi[2] : m.lo[2]);
    }
    float l[3], h[3];
    for (int k = 0; k < 3; ++k) {
      if (!(lo[k] <= hi[k])) lo[k] = hi[k] = 0.0;   // a mesh without triangles / non-finite transform: a point nobody hits
      // the tracer's world vertices are single-precision sums of four terms: four roundings of the largest one can get
      const double mag = std::fabs((double)M[k]) * std::max(std::fabs((double)m.lo[0]), std::fabs((double)m.hi[0])) +
                         std::fabs((double)M[4 + k]) * std::max(std::fabs((double)m.lo[1]), std::fabs((double)m.hi[1])) +
                         std::fabs((double)M[8 + k]) * std::max(std::fabs((double)m.lo[2]), std::fabs((double)m.hi[2])) + std::fabs((double)M[12 + k]);
      const double pad = 1e-5 * std::max({std::fabs(lo[k]), std::fabs(hi[k]), 1e-3}) + 1e-6 * (hi[k] - lo[k]) + (std::isfinite(mag) ? 4.8e-7 * mag : 0.0);
      l[k] = std::nextafterf((float)(lo[k] - pad), -INFINITY);
      h[k] = std::nextafterf((float)(hi[k] + pad), INFINITY);
    }
    blo[i] = make_float4(l[0], l[1], l[2], 0.0f);
    bhi[i] = make_float4(h[0], h[1], h[2], 0.0f);
  }
}

// how far from the origin the instances reach: the diagonal of their boxes' union plus its largest coordinate (TlasInstance::slack)
double instance_reach(const std::vector<float4>& blo, const std::vector<float4>& bhi) {
  double wlo[3] = {1e300, 1e300, 1e300}, whi[3] = {-1e300, -1e300, -1e300};
  for (size_t i = 0; i < blo.size(); ++i) {
    const float l[3] = {blo[i].x, blo[i].y, blo[i].z}, h[3] = {bhi[i].x, bhi[i].y, bhi[i].z};
    for (int k = 0; k < 3; ++k) {
      wlo[k] = std::min(wlo[k], (double)l[k]);
      whi[k] = std::max(whi[k], (double)h[k]);
    }
  }
  return std::sqrt((whi[0] - wlo[0]) * (whi[0] - wlo[0]) + (whi[1] - wlo[1]) * (whi[1] - wlo[1]) + (whi[2] - wlo[2]) * (whi[2] - wlo[2])) +
         std::max({std::fabs(wlo[0]), std::fabs(wlo[1]), std::fabs(wlo[2]), std::fabs(whi[0]), std::fabs(whi[1]), std::fabs(whi[2])});
}

bool host_instance_boxes_of(const SceneData& d, uint64_t budget, std::vector<float4>& lo, std::vector<float4>& hi, Error& err) {
  std::vector<glz_transform> transforms = d.transforms;
  if (transforms.empty()) transforms.push_back(identity_transform());   // as Scene::create
  if (!valid_geometry(d, transforms.size(), err)) return false;
  const std::vector<RTInstance> inst = rt_instances(d);
  std::vector<uint32_t> mesh_of, transform_of(inst.size());
  const std::vector<std::pair<uint32_t, uint32_t>> ranges = unique_meshes(inst, mesh_of);
  for (size_t i = 0; i < inst.size(); ++i) transform_of[i] = inst[i].transform_id;
  std::vector<std::vector<float>> pts = mesh_points(d, ranges);
  std::vector<InstanceBoxMesh> meshes(ranges.size());
  for (size_t m = 0; m < meshes.size(); ++m) {
    InstanceBoxMesh& b = meshes[m];
    for (int k = 0; k < 3; ++k) b.lo[k] = b.hi[k] = 0.0f;
    for (size_t p = 0; p + 2 < pts[m].size(); p += 3)
      for (int k = 0; k < 3; ++k) {
        b.lo[k] = p == 0 ? pts[m][p + k] : std::min(b.lo[k], pts[m][p + k]);
        b.hi[k] = p == 0 ? pts[m][p + k] : std::max(b.hi[k], pts[m][p + k]);
      }
    b.points = std::move(pts[m]);
  }
  host_instance_boxes(mesh_of, transform_of, meshes, transforms, budget, lo, hi);
  return true;
}

}  // namespace glz
