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

// The search of a piecewise-constant cdf of `size` entries as the kernels run it (device/shading.h: sample_cdf, the sky's row search):
// the upper bound of xi by bisection, the clamped offset and the position inside its step.  `bracket` null: the full search; otherwise
// it starts inside the bracket of xi wherever the device's does.  Returns the sample, *offset_out the row.
float sky_cdf_search(const float* cdf, uint32_t size, float xi, const uint16_t* bracket, uint32_t* offset_out);
// The bracket table of a cdf (device/types.h: kSkyBracketBuckets + 1 entries): entry b is where the full search's bisection ends for
// xi = b / kSkyBracketBuckets.  In a monotone cdf the search of any xi in [b, b + 1) / kSkyBracketBuckets ends inside [entry b, entry b + 1].
// A cdf with a descent or a NaN anywhere (there the end depends on the path the bisection takes), or of more entries than 16 bits count,
// gets the fall-back table: kSkyBracketFallback in every entry.  (glz_host_sky_bracket_table / glz_host_sky_cdf_search expose the two.)
void sky_bracket_table(const float* cdf, uint32_t size, uint16_t* table_out);

// Whether fresnel_conductor (device/shading.h) of a spectra pair -- n = ior, a = ior2abs2, 16 bins each -- is finite in every bin for
// every cosine |c| <= 2, so that its product with a zero metalness is a zero (kSpectraConductorFinite; glz_host_conductor_finite exposes
// it).  In double precision, per bin: n and a finite and at most 2^60 in magnitude, and the exact minima over |c| <= 2 of the routine's two
// denominators, a + 2nc + c^2 and a c^2 + 2nc + 1 (quadratics in c: the vertex and the two ends), at least 2^-10 M with
// M = |a| + 4|n| + 5.  4 M bounds every term, numerator and denominator (|c| <= 2: |a c^2| <= 4|a|); the float evaluation of a
// denominator is off by a few ulp of that, some 2^-19 M, five hundred times less than the margin, so the float denominators are normal and
// non-zero and the quotients stay below 2^12.  A condition, not a tuned value.  A NaN or infinite entry fails it.
bool conductor_finite(const float* ior, const float* ior2abs2);
// The pair of built-in metal `metal` (include/glz_tables.h) as a material record carries it: n, and n^2 + k^2 in float; false past the table
bool metal_spectra(uint32_t metal, float* ior_out, float* ior2abs2_out);

class ShadingTables {
 public:
  bool build_materials(hipStream_t st, const std::vector<glz_material>& materials, Error& err);
  // glz_debug_scene_set_spectra: gives one material's record spectra no built-in metal has and derives the tables again, flag included;
  // the next build_materials puts the material's own metal back
  bool debug_set_spectra(hipStream_t st, uint32_t material, const float* ior, const float* ior2abs2, Error& err);
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
  std::vector<uint16_t> h_sky_bracket;   // sky_bracket_table of the marginal cdf; on the device behind h_sky_marginal's floats (sky_bracket_offset)
  SkyHeader h_sky_header{};
  RTSky h_sky{};
  uint32_t lights_no = 0;   // lights.len() after reorder_lights (scene.rs:1549)

 private:
  bool upload_materials(hipStream_t st, Error& err);   // h_mat_compact and h_metal_spectra from h_materials, then the three device arrays
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
