// glz_host_denoise, glz_host_despeckle, glz_host_project_points and glz_host_reproject: the filter of glz_denoise_params and the firefly rejection of glz_despeckle_params (denoise.h)
// on the host cores, no device -- the reference the device kernels are compared with bit for bit.  Rows are dealt to a few threads; pixels of a pass do not interact, so the result does not depend on them.
#include <algorithm>
#include <thread>
#include <vector>

#include "denoise.h"
#include "reproject.h"

namespace glz {
namespace post {

namespace {
template <class F>
void for_rows(uint32_t h, uint32_t w, F f) {
  const uint32_t hw = std::thread::hardware_concurrency();
  const uint32_t want = (uint64_t)w * h < 65536u ? 1u : std::min<uint32_t>(std::min<uint32_t>(hw ? hw : 1u, 16u), h);
  if (want <= 1u) {
    for (uint32_t y = 0; y < h; ++y) f(y);
    return;
  }
  std::vector<std::thread> pool;
  for (uint32_t t = 0; t < want; ++t)
    pool.emplace_back([=] {
      for (uint32_t y = t; y < h; y += want) f(y);
    });
  for (auto& th : pool) th.join();
}

// the filter's passes on i_0 = src, which is `ping` or `pong`; the last one re-modulates into out
void filter_passes(uint32_t w, uint32_t h, const float4* src, float4* ping, float4* pong, const float4* aov0, const float4* aov1, const glz_denoise_params& P,
                   float4* out) {
  for (uint32_t k = 0; k < P.iterations; ++k) {
    const bool last = k + 1 == P.iterations;
    float4* dst = last ? out : (src == ping ? pong : ping);
    for_rows(h, w, [&](uint32_t y) {
      for (uint32_t x = 0; x < w; ++x) {
        float4 v = atrous_pixel(src, aov0, w, h, x, y, k, P);
        const size_t p = (size_t)y * w + x;
        if (last) v = remodulate(v, aov1[p], P.eps_albedo);
        dst[p] = v;
      }
    });
    src = dst;
  }
}
void demodulate_frame(uint32_t w, uint32_t h, const float4* result, const float4* aov1, float eps_albedo, float4* out) {
  for_rows(h, w, [&](uint32_t y) {
    for (size_t p = (size_t)y * w; p < (size_t)(y + 1) * w; ++p) out[p] = demodulate(result[p], aov1[p], eps_albedo);
  });
}
}  // namespace

void host_denoise(uint32_t w, uint32_t h, const float4* result, const float4* aov0, const float4* aov1, const glz_denoise_params& P, float4* out) {
  const size_t n = (size_t)w * h;
  std::vector<float4> ping(n), pong(P.iterations > 1u ? n : 0);
  demodulate_frame(w, h, result, aov1, P.eps_albedo, ping.data());
  filter_passes(w, h, ping.data(), ping.data(), pong.data(), aov0, aov1, P, out);
}

void host_despeckle(uint32_t w, uint32_t h, const float4* result, const float4* aov0, const float4* aov1, const glz_despeckle_params& D,
                    const glz_denoise_params& P, bool with_filter, float4* out) {
  const size_t n = (size_t)w * h;
  std::vector<float4> ping(n), pong(with_filter ? n : 0);
  demodulate_frame(w, h, result, aov1, P.eps_albedo, ping.data());
  float4* dst = with_filter ? pong.data() : out;
  for_rows(h, w, [&](uint32_t y) {
    for (uint32_t x = 0; x < w; ++x) {
      const float4 v = D.radius == 1u ? despeckle_pixel<1>(ping.data(), aov0, w, h, x, y, D.trim, D.ratio) : despeckle_pixel<2>(ping.data(), aov0, w, h, x, y, D.trim, D.ratio);
      const size_t p = (size_t)y * w + x;
      dst[p] = with_filter ? v : remodulate(v, aov1[p], P.eps_albedo);
    }
  });
  if (with_filter) filter_passes(w, h, pong.data(), ping.data(), pong.data(), aov0, aov1, P, out);
}

// ---- motion and reprojection (reproject.h) ----
void host_project_points(const ProjectConstants& C, uint32_t w, uint32_t h, const float* points3, size_t n, float* out3) {
  for (size_t i = 0; i < n; ++i) {
    const Projected r = project_point(C, (float)w, (float)h, points3[3 * i], points3[3 * i + 1], points3[3 * i + 2]);
    out3[3 * i] = r.fx;
    out3[3 * i + 1] = r.fy;
    out3[3 * i + 2] = r.z;
  }
}

void host_reproject(uint32_t w, uint32_t h, const float4* motion, const float4* color, const float4* aov0, const float4* aov1, const glz_reproject_params& P,
                    float4* out) {
  for_rows(h, w, [&](uint32_t y) {
    for (uint32_t x = 0; x < w; ++x) out[(size_t)y * w + x] = reproject_pixel(motion, color, aov0, aov1, w, h, x, y, P.depth_tolerance);
  });
}

}  // namespace post
}  // namespace glz
