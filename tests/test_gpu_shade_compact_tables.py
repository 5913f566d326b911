"""The shading kernels read a material from two derived tables -- its scalars from an 80-byte MatCompact record, its metal spectra from
the table of the scene's distinct pairs (device/types.h) -- which k_shade and k_path stage in LDS when they fit and read from memory
when they do not.  Every image has to keep every bit: HIP against the oracle as uint32, accumulator and result image, at 64 x 64 and
depth 4, in both launch modes:

  * the cube with each conductor family (Metal, Mirror, Uber with metalness > 0), of three different metals, next to Lambert faces;
  * the same with 60 materials of five metals, which fit k_shade's LDS area as compact records (5.7 KB) and did not as whole RTMaterial
    records (12.7 KB): the faces' records lie at the far end of a large staged table;
  * the same 60 materials with all 29 metals among them (8.8 KB) and 120 materials: these do not fit, the instantiation whose tables stay
    in memory.  Which case takes which instantiation follows from the tables' sizes, worked out here as the kernels' host side does
    (test_cases_are_on_the_side_of_the_lds_area_they_are_there_for);
  * after update_materials_and_lights turned a Lambert face into an Uber one of another metal, raised metalness_mul and made a metal
    face a mirror: the derived tables follow the RTMaterial array."""
import functools

import numpy as np
import pytest

import glaze_amd
from glaze_amd import abi
from glaze_amd.scene_desc import INSTANCE_DTYPE, MESH_DTYPE, make_camera, make_light, make_material
from glaze_amd.scenes import cube_scene
from oracle.pyoracle import OracleRenderer, OracleScene

pytestmark = pytest.mark.gpu

LAUNCHES, DEPTH, SIZE = 12, 4, (64, 64)
MODES = ("two_kernels", "path")
FACES = 6     # the cube's faces, one mesh and one material each


def bits(a):
    return np.nan_to_num(a, nan=-1.0).view(np.uint32)


def face_materials():
    """conductor lobes of three metals and Lambert, face by face"""
    return [make_material("metal", mtype=abi.MAT_METAL, metal=2, roughness_mul=0.3, diffuse=1),
            make_material("lambert a", diffuse=1, diffuse_mul=(230, 200, 180)),
            make_material("mirror", mtype=abi.MAT_MIRROR, metal=3),
            make_material("uber", mtype=abi.MAT_UBER, metal=7, metalness_mul=0.7, roughness_mul=0.4, diffuse=1, diffuse_mul=(200, 220, 240), ior=1.45),
            make_material("lambert b", diffuse=1, diffuse_mul=(180, 240, 190)),
            make_material("metal, default kind", mtype=abi.MAT_METAL, roughness_mul=0.5, anisotropy=0.3)]


def conductor_cube(n_materials, filler_metals):
    """the cube seen from inside, a light in it and one outside; its six faces use the LAST six of n_materials materials, so the
    records the kernels read lie at the far end of the tables; the fillers in front of them use `filler_metals` different metals"""
    desc = cube_scene()
    rng = np.random.default_rng(n_materials)
    desc.materials = desc.materials[:2]
    while len(desc.materials) < n_materials - FACES:
        i = len(desc.materials)
        desc.materials.append(make_material("filler%d" % i, mtype=abi.MAT_UBER if i % 3 == 0 else abi.MAT_LAMBERT, metal=i % filler_metals, diffuse=1,
                                            diffuse_mul=tuple(int(v) for v in rng.integers(60, 255, 3))))
    first = len(desc.materials)
    desc.materials += face_materials()
    desc.meshes = np.array([(k, first + k, 6 * k, 6) for k in range(FACES)], MESH_DTYPE)
    desc.instances = np.array([(k, 0) for k in range(FACES)], INSTANCE_DTYPE)
    desc.camera = make_camera(position=(0.2, 0.1, -0.3), target=(0.6, 0.4, 1.0), up=(0, 1, 0), fovx=np.float32(np.radians(np.float32(100.0))), near=1e-3, far=100.0)
    desc.lights.append(make_light(abi.LIGHT_SUN, "sun", direction=(0.2, -0.7, 0.4), intensity=0.8))
    return desc


def updated(desc):
    """what the update test turns the scene into: a Lambert face becomes an Uber one with metalness of a metal no material had, the
    Uber face more metallic, a metal face a mirror"""
    cur = desc.copy()
    first = len(cur.materials) - FACES
    cur.materials[first + 1].mtype = abi.MAT_UBER
    cur.materials[first + 1].metal = 11
    cur.materials[first + 1].metalness_mul = 0.9
    cur.materials[first + 1].roughness_mul = 0.25
    cur.materials[first + 3].metalness_mul = 1.0
    cur.materials[first + 5].mtype = abi.MAT_MIRROR
    return cur


# (materials, metals among the fillers): the six faces and the two defaults; 60 materials that fit the LDS area; 60 and 120 that do not
CASES = ((8, 1), (60, 2), (60, 29), (120, 29))
IDS = ["%d materials, %d filler metals" % c for c in CASES]
FIT = {(8, 1): True, (60, 2): True, (60, 29): False, (120, 29): False}
SHADE_LDS_TABLE_BYTES = 8192     # kShadeLdsTableBytes, device/shade_pixel.h


def table_bytes(desc, material_bytes):
    """SceneTables::bytes() of the scene: the materials at `material_bytes` each, a 128-byte MetalSpectra per distinct metal, a 112-byte
    RTLight per light (the scenes here have no area light, which would expand) and a 16-byte descriptor per texture"""
    metals = {int(m.metal) for m in desc.materials}
    return len(desc.materials) * material_bytes + 128 * len(metals) + 112 * len(desc.lights) + 16 * len(desc.textures)


@functools.lru_cache(maxsize=None)
def scene(case, after_update=False):
    desc = conductor_cube(*case)
    return updated(desc) if after_update else desc


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_cases_are_on_the_side_of_the_lds_area_they_are_there_for(case):
    """(no device needed; kept with the cases it describes)"""
    for after_update in (False, True):
        desc = scene(case, after_update)
        assert (table_bytes(desc, 80) <= SHADE_LDS_TABLE_BYTES) == FIT[case], table_bytes(desc, 80)
    if case == (60, 2):     # what the compact records bought: as whole RTMaterial records (the spectra inside, none beside) these did not fit
        assert len(scene(case).materials) * 208 > SHADE_LDS_TABLE_BYTES


@functools.lru_cache(maxsize=None)
def oracle_images(case, after_update=False):
    """(accumulator, result image) of the oracle after LAUNCHES launches, as uint32: computed once, shared by the launch modes"""
    o = OracleRenderer(OracleScene(scene(case, after_update)), *SIZE)
    o.set_depth(DEPTH)
    o.set_seed(3)
    o.step(LAUNCHES)
    hdr, result = bits(o.read_hdr()), bits(o.read_result())
    hdr.setflags(write=False)
    result.setflags(write=False)
    return hdr, result


def assert_same(r, want, what):
    hdr, result = want
    got = bits(r.read_hdr())
    assert np.array_equal(got, hdr), "%s: %d pixels of the accumulator differ" % (what, int((got != hdr).any(-1).sum()))
    got = bits(r.read_result())
    assert np.array_equal(got, result), "%s: %d pixels of the result image differ" % (what, int((got != result).any(-1).sum()))


def renderer(instance, case, mode):
    r = glaze_amd.RayTraceRenderer.new(instance, glaze_amd.RayTraceScene.from_desc(instance, scene(case)), *SIZE)
    r.set_launch_mode(mode)
    r.set_depth(DEPTH)
    r.set_seed(3)
    return r


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_conductors_next_to_lambert_keep_every_bit(instance, case, mode):
    r = renderer(instance, case, mode)
    r.step(LAUNCHES)
    assert_same(r, oracle_images(case), "%d materials, %d filler metals" % case)
    assert (r.read_result()[..., :3] > 0).any()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", ((60, 2), (120, 29)), ids=[IDS[1], IDS[3]])
def test_derived_tables_follow_an_update(instance, case, mode):
    r = renderer(instance, case, mode)
    r.step(3)
    cur = scene(case, True)
    r.update_materials_and_lights(cur.materials, cur.lights)
    r.step(LAUNCHES)
    assert_same(r, oracle_images(case, True), "%d materials, %d filler metals, after the update" % case)
    before, after = oracle_images(case), oracle_images(case, True)
    assert not np.array_equal(before[0], after[0])     # the update is one the image shows
