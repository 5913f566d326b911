"""The shading code skips memory requests and arithmetic whose result is known beforehand -- the accumulator's read-modify-write where
the sample adds exact zero (accumulate_shaded: four bytes mark the pixel), the sky texel of a light sample the BSDF rejects (fetched by
light_emission, k_shade only), the search over the sky's constant conditional cdf (written out in sample_light) -- and every image has
to keep every bit: HIP against the oracle as uint32, accumulator and result image, after 12 launches at depth 4, in both launch modes, at
72 x 40 and 200 x 136 (edge tiles, pixels outside the image, blocks that mix misses with hits).

The conditional cdf every lookup lands on is cdf[0] of the sky's first row, which distribution1d sets to 0: a render's xi, in [0, 1), is
always on its `cdf00 <= xi` side.  The other side (a negative xi, a NaN) is compared call by call through the light-sample hook."""
import functools

import numpy as np
import pytest

import glaze_amd
from glaze_amd import abi
from glaze_amd.scene_desc import INSTANCE_DTYPE, MESH_DTYPE, make_camera, make_light, make_material
from glaze_amd.scenes import cube_scene
from oracle.pyoracle import OracleRenderer, OracleScene

from conftest import MATTEST
from helpers import desc_from_oracle_parse

pytestmark = pytest.mark.gpu

LAUNCHES, DEPTH = 12, 4
SIZES = ((72, 40), (200, 136))
MODES = ("two_kernels", "path")


def bits(a):
    return np.nan_to_num(a, nan=-1.0).view(np.uint32)


def outside_camera():
    """the cube seen from outside: two of its faces, a third at a grazing angle, and the background around them"""
    return make_camera(position=(2.4, 1.7, -3.1), target=(0.0, 0.0, 0.0), up=(0, 1, 0), fovx=np.float32(np.radians(np.float32(55.0))), near=1e-3, far=100.0)


def noise_sky(height, width, seed):
    rng = np.random.default_rng(seed)
    px = rng.integers(1, 256, (height, width, 4), dtype=np.uint8)      # every texel another colour
    px[height // 3, :, :3] = 0                                          # and a black row: a plateau of the marginal cdf
    px[..., 3] = 255
    return px


def omni_cube():
    """The cube's own omni light sits inside it, the camera outside: a hit that picks it faces away from it (a BSDF pdf of 0: the update
    that adds exact zero).  A second omni light outside is behind the front face (z = -1) too and in front of the two others: the front
    face's pixels are marked in every launch and never added to, the others' get both kinds of update."""
    desc = cube_scene()
    desc.camera = outside_camera()
    desc.lights.append(make_light(abi.LIGHT_OMNI, "outside", position=(3.0, 2.5, 1.0), intensity=4.0))
    return desc


def sky_cube():
    desc = cube_scene(material_type=abi.MAT_UBER)
    desc.camera = outside_camera()
    desc.textures.append((abi.TEX_RGBA_SRGB, noise_sky(48, 96, 7), "noise sky"))
    desc.lights = [make_light(abi.LIGHT_SKY, "sky", resource_id=2, intensity=0.6, yaw=25, pitch=70, roll=5)]
    return desc


def sky_cube_tables_in_memory():
    """64 materials (13 KB of RTMaterial) and a sky of 1 500 rows: the k_shade whose tables and marginal cdf stay in memory"""
    desc = sky_cube()
    rng = np.random.default_rng(4)
    for i in range(61):
        desc.materials.append(make_material("m%d" % i, mtype=abi.MAT_UBER if i % 3 == 0 else abi.MAT_LAMBERT, diffuse=1,
                                            diffuse_mul=tuple(int(v) for v in rng.integers(60, 255, 3)), roughness_mul=0.3 + 0.01 * i))
    desc.meshes = np.array([(k, 3 + 10 * k, 6 * k, 6) for k in range(6)], MESH_DTYPE)     # a material per pair of faces
    desc.instances = np.array([(k, 0) for k in range(6)], INSTANCE_DTYPE)
    desc.textures[2] = (abi.TEX_RGBA_SRGB, noise_sky(1500, 16, 8), "tall noise sky")
    return desc


def sun_cube():
    desc = cube_scene()
    desc.camera = outside_camera()
    desc.lights = [make_light(abi.LIGHT_SUN, "sun", direction=(-0.5, -0.8, -0.3), intensity=1.2)]     # the front face (z = -1) is the shadow side
    return desc


SCENES = {"omni": (omni_cube, glaze_amd.Integrator.PATH_TRACE), "sky": (sky_cube, glaze_amd.Integrator.PATH_TRACE),
          "sky, tables in memory": (sky_cube_tables_in_memory, glaze_amd.Integrator.PATH_TRACE), "sun, direct": (sun_cube, glaze_amd.Integrator.DIRECT),
          "mattest": (lambda: desc_from_oracle_parse(MATTEST), glaze_amd.Integrator.PATH_TRACE)}
CASES = [(name, size) for name in ("omni", "sky", "sun, direct") for size in SIZES] + [("sky, tables in memory", SIZES[0]), ("mattest", (64, 64))]


@functools.lru_cache(maxsize=None)
def scene(name):
    return SCENES[name][0]()


def configure(x, name, seed):
    integrator = SCENES[name][1]
    x.set_integrator(integrator if isinstance(x, glaze_amd.RayTraceRenderer) else integrator.value)
    x.set_depth(DEPTH)
    x.set_seed(seed)
    if name == "mattest":
        x.set_exposure(scene(name).meta.exposure)


@functools.lru_cache(maxsize=None)
def oracle_images(name, size):
    """(accumulator, result image) of the oracle after LAUNCHES launches, as uint32: computed once, shared by the launch modes"""
    o = OracleRenderer(OracleScene(scene(name)), *size)
    configure(o, name, seed=3)
    o.step(LAUNCHES)
    hdr, result = bits(o.read_hdr()), bits(o.read_result())
    hdr.setflags(write=False)
    result.setflags(write=False)
    return hdr, result


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name,size", CASES, ids=["%s %dx%d" % (n, s[0], s[1]) for n, s in CASES])
def test_images_keep_every_bit(instance, name, size, mode):
    r = glaze_amd.RayTraceRenderer.new(instance, glaze_amd.RayTraceScene.from_desc(instance, scene(name)), *size)
    r.set_launch_mode(mode)
    configure(r, name, seed=3)
    r.step(LAUNCHES)
    hdr, result = oracle_images(name, size)
    got = bits(r.read_hdr())
    assert np.array_equal(got, hdr), "%d pixels of the accumulator differ" % int((got != hdr).any(-1).sum())
    got = bits(r.read_result())
    assert np.array_equal(got, result), "%d pixels of the result image differ" % int((got != result).any(-1).sum())
    if name == "omni":     # the case is there for the pixels that were marked and never added to: resolved (alpha 1), and exactly zero
        res = r.read_result()
        assert ((res[..., 3] == 1.0) & (res[..., :3] == 0).all(-1)).sum() > size[0] * size[1] // 50
        assert (res[..., :3] > 0).any() and (res[..., 3] == 0).any()     # next to pixels that were added to, and to misses


@pytest.mark.parametrize("mode", MODES)
def test_read_out_render_on_and_restart(instance, mode):
    """k_finalize after updates that only marked the pixel (the mark is all the resolve has of them), more launches on the resolved
    accumulator, and a restart in between -- against the oracle's plain sequence after every step"""
    name, size = "omni", (72, 40)
    r = glaze_amd.RayTraceRenderer.new(instance, glaze_amd.RayTraceScene.from_desc(instance, scene(name)), *size)
    r.set_launch_mode(mode)
    o = OracleRenderer(OracleScene(scene(name)), *size)
    for x in (r, o):
        configure(x, name, seed=9)
    for n in (1, 4, 2, 5):     # the first launch: every first hit behind the inner light is marked without ever having been added to
        r.step(n)
        o.step(n)
        assert np.array_equal(bits(r.read_hdr()), bits(o.read_hdr())), "accumulator after %d more launches" % n
        assert np.array_equal(bits(r.read_result()), bits(o.read_result())), "result image after %d more launches" % n
    r.restart()
    o.restart()
    for n in (3, 4):
        r.step(n)
        o.step(n)
        assert np.array_equal(bits(r.read_hdr()), bits(o.read_hdr())), "accumulator, %d launches after the restart" % n
        assert np.array_equal(bits(r.read_result()), bits(o.read_result())), "result image, %d launches after the restart" % n


def test_sky_sample_on_the_other_side_of_the_conditional_cdf(instance):
    """xi.x below cdf00 = 0 (and NaN, for which no comparison holds): the written-out search has to leave what sample_cdf left, u and
    with it the direction and the texel light_emission fetches -- call by call against the oracle, pdf first, then every field of the
    rows whose pdf is no NaN"""
    desc = scene("sky")
    o = OracleScene(desc)
    g = glaze_amd.RayTraceScene.from_desc(instance, desc)
    rng = np.random.default_rng(12)
    n = 512
    p = rng.uniform(-3.0, 3.0, (n, 3)).astype(np.float32)
    r3 = rng.random((n, 3), dtype=np.float32)
    tiny = np.float32(1e-45)
    r3[:128, 0] = -rng.random(128, dtype=np.float32)                       # below cdf00
    r3[128:136, 0] = [-0.0, 0.0, -tiny, tiny, -1.0, 1.0, np.nan, -np.inf]  # on it, next to it, and what never compares
    radius = float(desc.meta.scene_radius)
    got, want = g.debug_light_sample(0, p, r3, scene_radius=radius), o.light_sample(0, p, r3, scene_radius=radius)
    assert len(got) == len(want) == 4
    pdf_g, pdf_o = np.asarray(got[2], np.float32), np.asarray(want[2], np.float32)
    assert np.array_equal(bits(pdf_g), bits(pdf_o))
    live = ~np.isnan(pdf_o)
    assert live[:128].sum() > 100 and (pdf_o[:128][live[:128]] > 0).sum() > 50       # the rows below cdf00 are samples that count
    for a, b, what in zip(got, want, ("direction", "distance", "pdf", "emission")):
        a, b = np.asarray(a, np.float32)[live], np.asarray(b, np.float32)[live]
        assert np.array_equal(bits(a), bits(b)), what
