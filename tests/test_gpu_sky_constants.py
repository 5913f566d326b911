"""A sky sample reads the two words of the conditional tables it always lands on (sky_cond_cdf[0], sky_cond_values[0]) from the sky
header in the kernel arguments, and its row's marginal value and conditional integral as one pair of a per-row table
(DeviceScene::sky_rows) -- both made when the sky's distributions are built and rebuilt with them.  Checked against the oracle, bit for
bit:

  * the light-sample hook (k_debug_light_sample) call by call on skies of 16 x 8 and 64 x 32 texels, with xi.x on both sides of cdf00
    and the negative, NaN and infinite inputs of tests/test_gpu_shade_requests.py;
  * the same after the sky texture was replaced through refresh_binded_textures (another size: header constants and pair table rebuilt);
  * a 64 x 64 render lit by the sky alone, in both launch modes."""
import numpy as np
import pytest

import glaze_amd
from glaze_amd import abi
from glaze_amd.scene_desc import make_camera, make_light
from glaze_amd.scenes import cube_scene
from oracle.pyoracle import OracleRenderer, OracleScene

pytestmark = pytest.mark.gpu

SKIES = ((16, 8), (64, 32))     # width x height in texels


def bits(a):
    return np.nan_to_num(a, nan=-1.0).view(np.uint32)


def noise_sky(width, height, seed):
    rng = np.random.default_rng(seed)
    px = rng.integers(1, 256, (height, width, 4), dtype=np.uint8)      # every texel another colour: every row another pair
    px[height // 3, :, :3] = 0                                          # and a black row: a conditional integral of zero
    px[..., 3] = 255
    return px


def sky_cube(width, height, seed=7):
    """the cube seen from outside, the sky its only light"""
    desc = cube_scene(material_type=abi.MAT_UBER)
    desc.camera = make_camera(position=(2.4, 1.7, -3.1), target=(0.0, 0.0, 0.0), up=(0, 1, 0), fovx=np.float32(np.radians(np.float32(55.0))), near=1e-3, far=100.0)
    desc.textures.append((abi.TEX_RGBA_SRGB, noise_sky(width, height, seed), "noise sky"))
    desc.lights = [make_light(abi.LIGHT_SKY, "sky", resource_id=2, intensity=0.6, yaw=25, pitch=70, roll=5)]
    return desc


def sample_inputs():
    rng = np.random.default_rng(12)
    n = 512
    p = rng.uniform(-3.0, 3.0, (n, 3)).astype(np.float32)
    r3 = rng.random((n, 3), dtype=np.float32)
    tiny = np.float32(1e-45)
    r3[:128, 0] = -rng.random(128, dtype=np.float32)                       # below cdf00
    r3[128:136, 0] = [-0.0, 0.0, -tiny, tiny, -1.0, 1.0, np.nan, -np.inf]  # on it, next to it, and what never compares
    r3[136:144, 1] = [0.0, tiny, 1.0, -0.5, np.nan, 0.999999, 0.5, 0.25]   # the row search's ends: the first and the last pair
    return p, r3


def assert_samples_equal(g, o, radius, what):
    """g, o: the device scene and the oracle scene of the same description"""
    p, r3 = sample_inputs()
    got, want = g.debug_light_sample(0, p, r3, scene_radius=radius), o.light_sample(0, p, r3, scene_radius=radius)
    pdf_g, pdf_o = np.asarray(got[2], np.float32), np.asarray(want[2], np.float32)
    assert np.array_equal(bits(pdf_g), bits(pdf_o)), "%s: pdf" % what
    live = ~np.isnan(pdf_o)
    assert live[:128].sum() > 100 and (pdf_o[live] > 0).sum() > 200, what       # samples that count, on both sides of cdf00
    for a, b, field in zip(got, want, ("direction", "distance", "pdf", "emission")):
        a, b = np.asarray(a, np.float32)[live], np.asarray(b, np.float32)[live]
        assert np.array_equal(bits(a), bits(b)), "%s: %s" % (what, field)


@pytest.mark.parametrize("sky", SKIES, ids=["%dx%d" % s for s in SKIES])
def test_sky_samples_call_by_call(instance, sky):
    desc = sky_cube(*sky)
    assert_samples_equal(glaze_amd.RayTraceScene.from_desc(instance, desc), OracleScene(desc), float(desc.meta.scene_radius), "sky of %d x %d" % sky)


def test_sky_samples_after_the_sky_texture_is_replaced(instance):
    """refresh_binded_textures with a sky of another size and other texels: the samples are those of a scene created with it"""
    desc = sky_cube(16, 8)
    r = glaze_amd.RayTraceRenderer.new(instance, glaze_amd.RayTraceScene.from_desc(instance, desc), 64, 64)
    r.step(2)
    new = desc.copy()
    new.textures[2] = (abi.TEX_RGBA_SRGB, noise_sky(64, 32, 21), "another sky")
    r.refresh_binded_textures(new.textures)
    assert_samples_equal(r.scene, OracleScene(new), float(desc.meta.scene_radius), "after refresh_binded_textures")
    # and the renderer goes on with the new sky: a restart, then the images of a scene created with it
    r.set_depth(4)
    r.set_seed(3)
    r.restart()
    r.step(8)
    o = OracleRenderer(OracleScene(new), 64, 64)
    o.set_depth(4)
    o.set_seed(3)
    o.step(8)
    assert np.array_equal(bits(r.read_hdr()), bits(o.read_hdr()))


@pytest.mark.parametrize("mode", ("two_kernels", "path"))
def test_sky_only_render_keeps_every_bit(instance, mode):
    desc = sky_cube(64, 32)
    r = glaze_amd.RayTraceRenderer.new(instance, glaze_amd.RayTraceScene.from_desc(instance, desc), 64, 64)
    r.set_launch_mode(mode)
    o = OracleRenderer(OracleScene(desc), 64, 64)
    for x in (r, o):
        x.set_depth(4)
        x.set_seed(3)
        x.step(12)
    got, want = bits(r.read_hdr()), bits(o.read_hdr())
    assert np.array_equal(got, want), "%d pixels of the accumulator differ" % int((got != want).any(-1).sum())
    assert np.array_equal(bits(r.read_result()), bits(o.read_result()))
    assert (r.read_result()[..., :3] > 0).any()
