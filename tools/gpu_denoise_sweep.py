"""What the denoiser's default parameters were chosen on: the small Sponza-like atrium at 256 x 144, depth 8, 2 spp (seed 1) against 512 spp
of the unfiltered path with another seed; each parameter varied alone around the defaults.  Renders on the GPU, filters with the host
reference (the device filter equals it bit for bit).  Two figures per setting: MSE(denoised, converged) / MSE(noisy, converged) over all
pixels, and the same without the 1 % of pixels whose noisy error is largest (the first is set by fireflies of the 512-spp image).

Then the firefly rejection on the same scene (`despeckle` as the only argument runs this part alone): the reference R is the per-pixel,
per-channel median of nine independent 64-spp renders (seeds 101 .. 109) -- a median of means does not keep a firefly the way the single
512-spp image does.  ratio, trim and radius varied one at a time around the defaults: MSE(rejection + filter, R) / MSE(filter, R) at
2 spp over seeds 1 .. 8, all pixels.  Beside them, without a gate: the two figures above for rejection + filter against the 512-spp
image, the share of hit pixels the rule clamps at 2 spp and at 512 spp, and mean(despeckled) / mean(result), the energy it removes."""
import sys

sys.path.insert(0, ".")
import numpy as np
import glaze_amd
from glaze_amd.scenes import atrium_scene

inst = glaze_amd.RayTraceInstance.new()
if inst is None:
    raise SystemExit("no gfx950 device")
desc = atrium_scene(sponza_like=True, texture_size=64, sky_size=(64, 32))


def render(seed, spp):
    r = glaze_amd.RayTraceRenderer.new(inst, glaze_amd.RayTraceScene.from_desc(inst, desc), 256, 144)
    r.set_depth(8)
    r.set_seed(seed)
    r.draw(spp, want_image=False)
    return r, r.read_result()


only_despeckle = sys.argv[1:] == ["despeckle"]
conv_ren, conv_raw = render(987654321, 512)
conv = conv_raw
conv = conv[..., :3].astype(np.float64)
ren, noisy = render(1, 2)
aov0, aov1 = ren.read_aov(0), ren.read_aov(1)
nn = noisy[..., :3].astype(np.float64)
e_noisy = ((nn - conv) ** 2).sum(-1)
keep = e_noisy <= np.quantile(e_noisy, 0.99)
top = np.sort(e_noisy.ravel())[::-1]
print("MSE(noisy, converged): %.1f %% in the 10 pixels of largest error, %.1f %% in 100; converged max %.1f, mean %.3f" % (
    100 * top[:10].sum() / top.sum(), 100 * top[:100].sum() / top.sum(), conv.max(), conv.mean()))
for p in () if only_despeckle else ({}, dict(iterations=3), dict(iterations=4), dict(iterations=6), dict(sigma_color=1.0), dict(sigma_color=2.0), dict(sigma_color=8.0),
          dict(sigma_color=16.0), dict(sigma_depth=0.5), dict(sigma_depth=2.0), dict(sigma_depth=4.0), dict(normal_power_log2=0),
          dict(normal_power_log2=3), dict(normal_power_log2=4), dict(normal_power_log2=7), dict(eps_color=1e-4), dict(eps_color=1e-2)):
    e = ((glaze_amd.host_denoise(noisy, aov0, aov1, **p)[..., :3].astype(np.float64) - conv) ** 2).sum(-1)
    print("%-28s all pixels %.4f   without the 1 %% largest noisy errors %.4f" % (p or "defaults", e.mean() / e_noisy.mean(), e[keep].mean() / e_noisy[keep].mean()))


# ---- firefly rejection ----
SEEDS = range(1, 9)
R = np.median(np.stack([render(s, 64)[1][..., :3].astype(np.float64) for s in range(101, 110)]), axis=0)
frames = []
for s in SEEDS:
    rs, f = render(s, 2)
    frames.append((f, rs.read_aov(0), rs.read_aov(1)))
base = [((glaze_amd.host_denoise(*f)[..., :3].astype(np.float64) - R) ** 2).mean() for f in frames]
print("reference R: median of nine 64-spp renders; max %.2f, mean %.3f (the 512-spp image: max %.1f, mean %.3f)" % (R.max(), R.mean(), conv.max(), conv.mean()))
print("MSE(filter alone, R) over seeds 1 .. 8: %s" % ", ".join("%.5f" % b for b in base))
for p in ({}, dict(ratio=4.0), dict(ratio=6.0), dict(ratio=12.0), dict(ratio=16.0), dict(trim=0), dict(trim=1), dict(trim=3), dict(radius=1)):
    ratios = [((glaze_amd.host_despeckle(*f, with_filter=True, **p)[..., :3].astype(np.float64) - R) ** 2).mean() / b for f, b in zip(frames, base)]
    print("%-16s MSE(rejection + filter, R) / MSE(filter, R): %s   worst %.4f" % (p or "defaults", ", ".join("%.4f" % v for v in ratios), max(ratios)))
# against the single 512-spp image, as the filter's figures above (seed 1)
e = ((glaze_amd.host_despeckle(noisy, aov0, aov1, with_filter=True)[..., :3].astype(np.float64) - conv) ** 2).sum(-1)
print("rejection + filter against the 512-spp image (seed 1): all pixels %.4f   without the 1 %% largest noisy errors %.4f" % (
    e.mean() / e_noisy.mean(), e[keep].mean() / e_noisy[keep].mean()))
for name, (res, a0, a1) in (("2 spp (seed 1)", (noisy, aov0, aov1)), ("512 spp", (conv_raw, conv_ren.read_aov(0), conv_ren.read_aov(1)))):
    out = glaze_amd.host_despeckle(res, a0, a1)
    untouched = glaze_amd.host_despeckle(res, a0, a1, ratio=3e38)
    hit = np.isfinite(a0[..., 3])
    moved = (out.view(np.uint32) != untouched.view(np.uint32)).any(-1)
    print("%s: %d of %d hit pixels clamped (%.3f %%); mean(despeckled) / mean(result) = %.4f; largest value %.1f -> %.1f" % (
        name, moved.sum(), hit.sum(), 100.0 * moved.sum() / hit.sum(), out[..., :3].astype(np.float64).mean() / res[..., :3].astype(np.float64).mean(),
        res[..., :3].max(), out[..., :3].max()))
