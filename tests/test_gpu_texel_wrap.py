"""The sampler's wrap of a power-of-two size (i & (n - 1), device/shading.h bilinear_level) and its 24-bit tile-row multiply
(texel_address), on the device: glz_debug_sample_texture against the oracle's sampler, bit for bit.

Sizes whose two sides are powers of two take the new wrap -- 2 x 2, 8 x 4 (one RGBA tile), 16 x 8 (one gray tile; two RGBA tiles each
way); 1 x 1 is the inline texel and wraps nothing -- and sizes with one side that is not keep the remainder for both: 3 x 5, 12 x 7,
16 x 9, 9 x 16.  All three formats.  Coordinates: a grid over [-3, 3]^2, values exactly on texel borders, +-2^23 / width (where the int
path ends) with its float neighbours, 1e10, +-inf and NaN.  In the launches with a footprint the lanes fetch different mip levels of one
texture, so one launch mixes power-of-two and other sizes from lane to lane (16 x 9 -> 8 x 4 -> 4 x 2; 12 x 7 -> 6 x 3 -> 3 x 1)."""
import numpy as np
import pytest

import glaze_amd
from glaze_amd import abi
from oracle.pyoracle import OracleScene

from test_texture_sampler import assert_same, textured_desc, texture_pixels

pytestmark = pytest.mark.gpu

POW2 = [(1, 1), (2, 2), (8, 4), (16, 8)]
OTHER = [(3, 5), (12, 7), (16, 9), (9, 16)]
FORMATS = (abi.TEX_RGBA_SRGB, abi.TEX_RGBA_NORM, abi.TEX_GRAY)
TEXTURES = [(w, h, fmt) for (w, h) in POW2 + OTHER for fmt in FORMATS]


def coordinates(w, h):
    """(n, 2) float32"""
    def axis(n):
        grid = np.linspace(-3.0, 3.0, 49)
        borders = np.arange(-2 * n, 2 * n + 1) / n                  # exactly on texel borders ...
        centres = (np.arange(-n, 2 * n) + 0.5) / n                  # ... and centres, where the weight is 0 and the index is the texel's
        edge = np.float32(2.0 ** 23 / n)
        near = [edge, np.nextafter(edge, np.float32(0)), np.nextafter(edge, np.float32(np.inf))]
        near = np.array(near + [-x for x in near], np.float32)
        far = np.array([1e10, -1e10, np.inf, -np.inf, np.nan], np.float32)
        return np.concatenate([grid, borders, centres]).astype(np.float32), np.concatenate([near, far])
    au, su = axis(w)
    av, sv = axis(h)
    rng = np.random.default_rng(w * 100 + h)
    pairs = [np.stack(np.meshgrid(au, av), -1).reshape(-1, 2),
             np.stack(np.meshgrid(su, av[::7]), -1).reshape(-1, 2), np.stack(np.meshgrid(au[::7], sv), -1).reshape(-1, 2),
             np.stack(np.meshgrid(su, sv), -1).reshape(-1, 2), rng.uniform(-3, 3, (2000, 2))]
    return np.ascontiguousarray(np.concatenate(pairs).astype(np.float32))


@pytest.fixture(scope="module")
def scenes(instance):
    desc = textured_desc([(fmt, texture_pixels(w, h, fmt, 50 + i)) for i, (w, h, fmt) in enumerate(TEXTURES)])
    return glaze_amd.RayTraceScene.from_desc(instance, desc), OracleScene(desc)


@pytest.mark.parametrize("k", range(len(TEXTURES)), ids=["%dx%d-fmt%d" % t for t in TEXTURES])
def test_level_0_equals_the_oracle(scenes, k):
    gpu, sc = scenes
    w, h, fmt = TEXTURES[k]
    uv = coordinates(w, h)
    assert_same(gpu.debug_sample_texture(k + 1, uv), sc.sample_texture(k + 1, uv), "%d x %d, format %d" % (w, h, fmt))


def test_a_texture_of_2_to_the_24_tile_rows_is_refused(instance):
    """what makes the 24-bit multiply exact: the tile row stays below 2^24 because no such texture is taken (a gray column of 2^27 texels,
    128 MiB: 2^24 tile rows of 8; its 2 GiB of tiles would fit the pool)"""
    desc = textured_desc([(abi.TEX_GRAY, np.zeros((1 << 27, 1), np.uint8))])
    with pytest.raises(abi.GlazeError, match="tile rows") as err:
        glaze_amd.RayTraceScene.from_desc(instance, desc)
    assert err.value.status == abi.E_UNSUPPORTED


@pytest.mark.parametrize("k", [k for k, (w, h, _) in enumerate(TEXTURES) if (w, h) in ((16, 9), (9, 16), (12, 7), (16, 8))],
                         ids=lambda k: "%dx%d-fmt%d" % TEXTURES[k])
def test_lanes_of_one_launch_at_levels_of_either_kind(scenes, k):
    """neighbouring lanes at level 0, between 0 and 1, at 1, between 1 and 2, ...: a fractional level fetches both of its levels"""
    gpu, sc = scenes
    w, h, fmt = TEXTURES[k]
    uv = coordinates(w, h)[:6000]
    n = len(uv)
    base0 = -0.5 * np.log2(w * h)                                    # the lod_base of level 0 exactly
    fp = np.zeros((n, 4), np.float32)
    fp[:, 0] = base0 + (np.arange(n) % 9) * 0.5                      # levels 0, 0.5, 1 .. 4 from lane to lane
    fp[:, 3] = 1
    assert_same(gpu.debug_sample_texture(k + 1, uv, fp), sc.sample_texture(k + 1, uv, fp), "%d x %d, format %d, mixed levels" % (w, h, fmt))
