"""k_shade's residency paths against the oracle, bit for bit.

launch_shade picks an instantiation of k_shade by whether the material / light / texture-descriptor tables fit their 8 KB LDS copy
(38 materials) and whether the sky's marginal cdf fits its own (1 087 rows): the copies are read with LDS instructions, what does not fit
with global loads.  All four combinations render a small open atrium -- Lambert and Uber materials with a texture each, a sun and a sky
-- for 12 launches at depth 4, in the two-kernel launch mode (a frame this small would otherwise run as k_path); a second frame size puts
8 x 8 pixel blocks partly outside the image."""
import numpy as np
import pytest

import glaze_amd
from glaze_amd.scenes import atrium_scene
from oracle.pyoracle import OracleRenderer, OracleScene

pytestmark = pytest.mark.gpu

LDS_TABLE_MATERIALS, LDS_SKY_ROWS = 38, 1087


def scene(many_materials, tall_sky):
    desc = atrium_scene(detail=0.02, texture_size=32, sky_size=(8, 1100) if tall_sky else (16, 64))
    if many_materials:
        # every material once more; every other mesh takes the copy, so records on both sides of the 8 KB mark are read
        n = len(desc.materials)
        desc.materials = desc.materials + [m for m in desc.copy().materials[1:]]
        odd = (np.arange(desc.meshes.shape[0]) % 2) == 1
        desc.meshes["material"][odd] += n - 1
    assert (len(desc.materials) > LDS_TABLE_MATERIALS) == many_materials
    assert (desc.textures[-1][1].shape[0] > LDS_SKY_ROWS) == tall_sky
    return desc


@pytest.mark.parametrize("many_materials, tall_sky, size", [
    (False, False, (64, 48)), (False, False, (60, 45)), (True, False, (64, 48)), (False, True, (64, 48)), (True, True, (64, 48)), (True, True, (60, 45))],
    ids=["resident", "resident 60x45", "tables in memory", "sky in memory", "both in memory", "both in memory 60x45"])
def test_k_shade_residency_paths_equal_the_oracle(instance, many_materials, tall_sky, size):
    desc = scene(many_materials, tall_sky)
    w, h = size
    r = glaze_amd.RayTraceRenderer.new(instance, glaze_amd.RayTraceScene.from_desc(instance, desc), w, h)
    r.set_launch_mode("two_kernels")
    o = OracleRenderer(OracleScene(desc), w, h)
    for x in (r, o):
        x.set_depth(4)
        x.set_seed(3)
        x.step(12)
    g, c = r.read_hdr(), o.read_hdr()
    assert (c[..., 3] == 12.0).all() and (c[..., :3] > 0.0).any(-1).mean() > 0.5        # the scene is lit
    assert np.array_equal(np.isnan(g), np.isnan(c))
    same = (g.view(np.uint32) == c.view(np.uint32)) | np.isnan(c)
    assert same.all(), "%d pixels differ from the oracle" % int((~same).any(-1).sum())
    gr, cr = r.read_result(), o.read_result()
    assert ((gr.view(np.uint32) == cr.view(np.uint32)) | (np.isnan(gr) & np.isnan(cr))).all()
