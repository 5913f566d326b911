// The tables the shading kernels read: RTMaterial records, RTLight records, and the sky with its sampling distributions.  The device
// buffers are private; describe() names them in the kernels' view.  The host mirrors are public: the debug read-back compares them
// with the oracle.
#pragma once
#include <vector>

#include "hip_util.h"
#include "kernels.h"
#include "parser.h"

namespace glz {

// The sky's per-row table (DeviceScene::sky_rows): pair y = (marginal_values[y], conditional_integrals[y]), the same floats interleaved
// (glz_host_sky_row_pairs exposes it).
void sky_row_pairs(const float* marginal_values, const float* conditional_integrals, size_t n, float* pairs_out);

class ShadingTables {
 public:
  bool build_materials(hipStream_t st, const std::vector<glz_material>& materials, Error& err);
  // n_instances: the instances the device got (an area light names one of them)
  bool build_lights_and_sky(hipStream_t st, const SceneData& data, size_t n_instances, Error& err);
  void forget_sky_distribution() { sky_distribution_tex_ = 0xFFFFFFFFu; }   // the sky map's texels may have changed: rebuilt by the next build
  // some material carries an opacity map: which k_trace runs (launch_trace), the one without alpha code or the one with the alpha phase
  bool has_non_opaque() const;
  const RTMaterial* materials() const { return d_materials_.ptr; }   // device (the hierarchy build and the alpha records read them)
  // materials, lights, sky*, has_non_opaque and their counts
  void describe(DeviceScene& dev) const;

  std::vector<RTMaterial> h_materials;
  std::vector<MatCompact> h_mat_compact;   // h_materials without the metal spectra, rebuilt with them ...
  std::vector<MetalSpectra> h_metal_spectra;   // ... and their distinct spectra pairs (MatCompact::spectra)
  std::vector<RTLight> h_lights;
  std::vector<float> h_sky_marginal;
  std::vector<float> h_sky_rows;   // per row (marginal value, conditional integral), sky_row_pairs of h_sky_marginal's two last parts
  SkyHeader h_sky_header{};
  RTSky h_sky{};
  uint32_t lights_no = 0;   // lights.len() after reorder_lights (scene.rs:1549)

 private:
  DeviceBuffer<RTMaterial> d_materials_;
  DeviceBuffer<MatCompact> d_mat_compact_;
  DeviceBuffer<MetalSpectra> d_metal_spectra_;
  DeviceBuffer<RTLight> d_lights_;
  DeviceBuffer<float> d_sky_marginal_, d_sky_cond_values_, d_sky_cond_cdf_;
  DeviceBuffer<float2> d_sky_rows_;
  uint32_t sky_distribution_tex_ = 0xFFFFFFFFu;   // the texture the sky's distributions were computed from
  uint32_t sky_w_ = 0, sky_h_ = 0;
};

}  // namespace glz
