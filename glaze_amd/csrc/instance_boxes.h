// The instance boxes of a two-level top level, on the host: which instances a scene description gives the device, the distinct
// meshes they draw, and the rule for each instance's world box.  Host code only -- nothing here calls the HIP runtime, so the file
// builds and runs on its own (tools/sanitize).  The device side of the same rule is kernels_tlas.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <utility>
#include <vector>

#include "device/types.h"
#include "glaze_abi.h"
#include "parser.h"

namespace glz {

// Past this many point transforms, the remaining instances (in instance order) take the eight corners of their mesh's box.
constexpr uint64_t kExactBoxBudget = 50000000ull;
struct InstanceBoxMesh {
  float lo[3], hi[3];          // the mesh's object box
  std::vector<float> points;   // xyz of the distinct vertices the mesh references
};
const glz_mesh* mesh_by_id(const SceneData& d, uint32_t id);   // meshes are indexed by id, the last one with an id wins; null: no such mesh
std::vector<RTInstance> rt_instances(const SceneData& d);      // the instances the device gets (dangling ones dropped)
// The distinct index ranges (offset, count) the instances draw, in first-use order (it fixes tri_base, node_base and the order in which
// the exact-box budget is spent), and which of them each instance uses.
std::vector<std::pair<uint32_t, uint32_t>> unique_meshes(const std::vector<RTInstance>& instances, std::vector<uint32_t>& mesh_of);
// References inside the geometry, so that nothing indexes out of bounds: index ranges, vertex indices, transform ids
bool valid_geometry(const SceneData& d, size_t n_transforms, Error& err);
// xyz of the distinct vertices each index range (offset, count) references, in first-use order
std::vector<std::vector<float>> mesh_points(const SceneData& d, const std::vector<std::pair<uint32_t, uint32_t>>& ranges);
// which instances take the exact box: in instance order, while the points spent stay within `budget`
std::vector<uint8_t> exact_box_instances(const std::vector<uint32_t>& mesh_of, const std::vector<uint64_t>& mesh_point_count, uint64_t budget);
// The host rule: instance i = mesh mesh_of[i] under transforms[transform_of[i]]; the f64 world AABB of the mesh's points (or of the
// corners of its box), padded for the tracer's single-precision world vertices and widened by one ulp outwards.  Non-finite
// transforms give a padded box around the origin.
void host_instance_boxes(const std::vector<uint32_t>& mesh_of, const std::vector<uint32_t>& transform_of, const std::vector<InstanceBoxMesh>& meshes,
                         const std::vector<glz_transform>& transforms, uint64_t budget, std::vector<float4>& lo, std::vector<float4>& hi);
double instance_reach(const std::vector<float4>& lo, const std::vector<float4>& hi);
// The host rule on a scene description, no device: the meshes' boxes are the min / max of their vertices (a scene's own build takes
// its mesh hierarchies' root boxes).  One box per instance that names an existing mesh.
bool host_instance_boxes_of(const SceneData& d, uint64_t budget, std::vector<float4>& lo, std::vector<float4>& hi, Error& err);

}  // namespace glz
