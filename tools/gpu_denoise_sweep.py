"""What the denoiser's default parameters were chosen on: the small Sponza-like atrium at 256 x 144, depth 8, 2 spp (seed 1) against 512 spp
of the unfiltered path with another seed; each parameter varied alone around the defaults.  Renders on the GPU, filters with the host
reference (the device filter equals it bit for bit).  Two figures per setting: MSE(denoised, converged) / MSE(noisy, converged) over all
pixels, and the same without the 1 % of pixels whose noisy error is largest (the first is set by fireflies of the 512-spp image)."""
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


_, conv = render(987654321, 512)
conv = conv[..., :3].astype(np.float64)
ren, noisy = render(1, 2)
aov0, aov1 = ren.read_aov(0), ren.read_aov(1)
nn = noisy[..., :3].astype(np.float64)
e_noisy = ((nn - conv) ** 2).sum(-1)
keep = e_noisy <= np.quantile(e_noisy, 0.99)
top = np.sort(e_noisy.ravel())[::-1]
print("MSE(noisy, converged): %.1f %% in the 10 pixels of largest error, %.1f %% in 100; converged max %.1f, mean %.3f" % (
    100 * top[:10].sum() / top.sum(), 100 * top[:100].sum() / top.sum(), conv.max(), conv.mean()))
for p in ({}, dict(iterations=3), dict(iterations=4), dict(iterations=6), dict(sigma_color=1.0), dict(sigma_color=2.0), dict(sigma_color=8.0),
          dict(sigma_color=16.0), dict(sigma_depth=0.5), dict(sigma_depth=2.0), dict(sigma_depth=4.0), dict(normal_power_log2=0),
          dict(normal_power_log2=3), dict(normal_power_log2=4), dict(normal_power_log2=7), dict(eps_color=1e-4), dict(eps_color=1e-2)):
    e = ((glaze_amd.host_denoise(noisy, aov0, aov1, **p)[..., :3].astype(np.float64) - conv) ** 2).sum(-1)
    print("%-28s all pixels %.4f   without the 1 %% largest noisy errors %.4f" % (p or "defaults", e.mean() / e_noisy.mean(), e[keep].mean() / e_noisy[keep].mean()))
