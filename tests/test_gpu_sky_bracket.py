"""The sky's row search that starts inside the bracket of its xi (device/shading.h sample_cdf, the table of shading_tables.cpp), on the
device: the light-sample hook call by call against the oracle, bit for bit.  The hook stages the marginal cdf and its bracket table in LDS
the way k_shade does when the cdf fits (skies of 1, 2, 3, 17, 64 and 1 087 rows: the smallest, the sizes of the host test, the largest
that fits) and searches a taller sky's cdf in memory, all of it (1 100 rows).  4 096 samples each: xi.y at every cdf value and its two
float neighbours, 0, the float below 1, 1, -0.5 and NaN (3 308 values for the tallest sky), the rest random."""
import numpy as np
import pytest

import glaze_amd
from glaze_amd import abi
from glaze_amd.scene_desc import make_camera, make_light
from glaze_amd.scenes import cube_scene
from oracle.pyoracle import OracleScene

from sky_bracket_cases import search_points

pytestmark = pytest.mark.gpu

ROWS = (1, 2, 3, 17, 64, 1087, 1100)
WIDTH = 4
N = 4096


def bits(a):
    return np.nan_to_num(np.asarray(a, np.float32), nan=-1.0).view(np.uint32)


def sky_of(rows, seed):
    """every texel another colour, with runs of black rows: plateaus of the marginal cdf"""
    rng = np.random.default_rng(seed)
    px = rng.integers(1, 256, (rows, WIDTH, 4), dtype=np.uint8)
    if rows >= 17:
        px[rows // 3: rows // 3 + 3, :, :3] = 0
        px[rows - 2:, :, :3] = 0
        bright = rng.integers(0, rows, max(1, rows // 40))
        dark = np.setdiff1d(np.arange(rows), bright)
        px[dark, :, :3] //= 8                                   # a few rows carry most of the light: narrow and wide brackets
    px[..., 3] = 255
    return px


def sky_desc(rows):
    desc = cube_scene(material_type=abi.MAT_LAMBERT)
    desc.camera = make_camera(position=(2.4, 1.7, -3.1), target=(0.0, 0.0, 0.0), up=(0, 1, 0), fovx=np.float32(np.radians(np.float32(55.0))), near=1e-3, far=100.0)
    desc.textures.append((abi.TEX_RGBA_SRGB, sky_of(rows, 30 + rows), "sky of %d rows" % rows))
    desc.lights = [make_light(abi.LIGHT_SKY, "sky", resource_id=2, intensity=0.7, yaw=10, pitch=40, roll=0)]
    return desc


@pytest.mark.parametrize("rows", ROWS)
def test_sky_samples_equal_the_oracle(instance, rows):
    desc = sky_desc(rows)
    g, o = glaze_amd.RayTraceScene.from_desc(instance, desc), OracleScene(desc)
    cdf = g.debug_sky()[40:40 + rows + 1].copy()
    assert cdf[0] == 0.0 and (np.diff(cdf) >= 0).all() and cdf[-1] > 0.0
    points = search_points(cdf)                      # 3 (rows + 1) + 5 values: 3 308 for the tallest sky
    assert len(points) <= N
    rng = np.random.default_rng(rows)
    r3 = rng.random((N, 3), dtype=np.float32)        # the rest of the 4 096 stay random
    r3[:len(points), 1] = points
    p = rng.uniform(-3.0, 3.0, (N, 3)).astype(np.float32)
    radius = float(desc.meta.scene_radius)
    got, want = g.debug_light_sample(0, p, r3, scene_radius=radius), o.light_sample(0, p, r3, scene_radius=radius)
    pdf_o = np.asarray(want[2], np.float32)
    assert np.array_equal(bits(got[2]), bits(pdf_o)), "pdf"
    live = ~np.isnan(pdf_o)
    assert (pdf_o[live] > 0).sum() > N // 4          # samples that count
    for a, b, field in zip(got, want, ("direction", "distance", "pdf", "emission")):
        assert np.array_equal(bits(np.asarray(a, np.float32)[live]), bits(np.asarray(b, np.float32)[live])), field
