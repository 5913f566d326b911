"""k_shade hands the spectrum bsdf_eval made of a Lambert hit's tint to bsdf_sample (device/shade_pixel.h, StagedState::kHandLambert)
instead of converting the same colour a second time; k_path keeps the two conversions.  Both must leave the oracle's image: a 96 x 64
render of a box whose faces and floor are the six BSDF families -- so that waves hold Lambert lanes next to lanes of every other kind,
hits whose evaluation ran and hits whose light sample was empty -- under a sun and a sky, depth 8, 40 launches, equal to the oracle as
uint32 in both launch modes.  (The sky's row search, bracketed in both kernels, is in every one of those sky samples too.)"""
import functools

import numpy as np
import pytest

import glaze_amd
from glaze_amd import abi
from glaze_amd.scene_desc import INSTANCE_DTYPE, MESH_DTYPE, make_camera, make_light, make_material, make_meta
from glaze_amd.scenes import cube_scene
from oracle.pyoracle import OracleRenderer, OracleScene

SIZE, DEPTH, LAUNCHES = (96, 64), 8, 40
MODES = ("two_kernels", "path")
TOP, FRONT, LEFT, BOTTOM, RIGHT, BACK = range(6)     # the cube's faces in index order, by their normals: +y, +z, -x, -y, +x, -z
TEX_SKY = 2


def sky_pixels():
    rng = np.random.default_rng(77)
    px = rng.integers(1, 256, (48, 32, 4), dtype=np.uint8)
    px[10:14, :, :3] = 0
    px[30, :, :3] = 255
    px[..., 3] = 255
    return px


@functools.lru_cache(maxsize=None)
def box_desc():
    desc = cube_scene()
    desc.textures += [(abi.TEX_RGBA_SRGB, sky_pixels(), "sky")]
    first = len(desc.materials)
    desc.materials += [make_material("lambert wall", mtype=abi.MAT_LAMBERT, diffuse=1, diffuse_mul=(230, 200, 180)),
                       make_material("uber wall", mtype=abi.MAT_UBER, roughness_mul=0.5, ior=1.5, diffuse=1, metal=1, metalness_mul=0.3, diffuse_mul=(180, 240, 190)),
                       make_material("metal top", mtype=abi.MAT_METAL, roughness_mul=0.4, metal=2, anisotropy=0.2),
                       make_material("frosted wall", mtype=abi.MAT_FROSTED, roughness_mul=0.3, ior=1.5),
                       make_material("glass wall", mtype=abi.MAT_GLASS, ior=1.45),
                       make_material("mirror wall", mtype=abi.MAT_MIRROR, metal=0),
                       make_material("lambert floor", mtype=abi.MAT_LAMBERT, diffuse=1, diffuse_mul=(220, 220, 220))]
    lambert, uber, metal, frosted, glass, mirror, floor_mat = range(first, first + 7)
    faces = ((FRONT, lambert), (RIGHT, uber), (TOP, metal), (LEFT, frosted), (BACK, glass), (BOTTOM, mirror), (TOP, floor_mat))
    desc.meshes = np.array([(k, mat, 6 * face, 6) for k, (face, mat) in enumerate(faces)], MESH_DTYPE)
    floor = np.diag([4.0, 1.0, 4.0, 1.0])
    floor[1, 3] = -2.0
    desc.transforms = np.ascontiguousarray(np.stack([np.eye(4, dtype=np.float32).reshape(16), floor.astype(np.float32).T.reshape(16)]))
    desc.instances = np.array([(k, 1 if k == len(faces) - 1 else 0) for k in range(len(faces))], INSTANCE_DTYPE)
    desc.camera = make_camera(position=(2.2, 1.6, 2.6), target=(0.0, -0.2, 0.0), up=(0, 1, 0), fovx=np.float32(np.radians(np.float32(70.0))), near=1e-3, far=100.0)
    desc.meta = make_meta(centre=(0, 0, 0), radius=6.0, exposure=1.0)
    desc.lights = [make_light(abi.LIGHT_SUN, "sun", direction=(-0.4, -0.7, -0.5), intensity=0.8),
                   make_light(abi.LIGHT_SKY, "sky", resource_id=TEX_SKY, intensity=0.5, yaw=20, pitch=10)]
    return desc


def bits(a):
    return np.nan_to_num(a, nan=-1.0).view(np.uint32)


@functools.lru_cache(maxsize=None)
def oracle_images():
    o = OracleRenderer(OracleScene(box_desc()), *SIZE)
    o.set_depth(DEPTH)
    o.set_seed(5)
    o.step(LAUNCHES)
    hdr, result = bits(o.read_hdr()), bits(o.read_result())
    hdr.setflags(write=False)
    result.setflags(write=False)
    return hdr, result


def test_the_oracle_image_shows_the_scene():
    hdr, result = oracle_images()
    lit = (result.view(np.float32)[..., :3] > 0).any(-1)
    assert lit.mean() > 0.5


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_render_equals_the_oracle(instance, mode):
    r = glaze_amd.RayTraceRenderer.new(instance, glaze_amd.RayTraceScene.from_desc(instance, box_desc()), *SIZE)
    r.set_launch_mode(mode)
    r.set_depth(DEPTH)
    r.set_seed(5)
    r.step(LAUNCHES)
    assert r.launch_mode() == mode
    hdr, result = oracle_images()
    got = bits(r.read_hdr())
    assert np.array_equal(got, hdr), "%s: %d pixels of the accumulator differ" % (mode, int((got != hdr).any(-1).sum()))
    got = bits(r.read_result())
    assert np.array_equal(got, result), "%s: %d pixels of the result image differ" % (mode, int((got != result).any(-1).sum()))
