"""The Uber specular lobe skips the conductor Fresnel term where a zero metalness multiplies it (device/shading.h: uber_specular_value):
the pair of spectra is conductor_finite (test_conductor_flag_host.py), the computed metalness is 0 and the cosine is within |c| <= 2.
The skip must not move a bit, and a lane that fails any of the three conditions must run the whole term.

Call by call, through the BSDF hooks of test_gpu_shading_routines.py and by its rule (same bits, or NaN on both sides; the pdf on every
row, value and direction where the oracle's pdf is > 0), N calls per case:

  * metalness_mul = 0 on a flagged pair (gold): every lane skips;
  * metalness_mul = 0 on a built-in pair WITHOUT the flag (germanium): every lane runs the term;
  * metalness_mul = 0.5: the product is not zero;
  * metalness_mul = 1 with a metalness map whose texels are 0 and 255: calls at the one texel skip, calls at the other do not;
  * the inputs hold wi = -wo (the half vector is NaN, and so is the cosine: the comparison fails, the term runs), wi = (wo.x, wo.y, -wo.z)
    and directions in the horizon (the half vector lies in the surface, the cosine is exactly 0), both signs of wo.z, and the lobe
    choice xi on both sides of 0.5, at 0.5 and at its lower neighbour.

The all-zero pair (the denominator of the term is c^2: 0 / 0 at c = 0) is no built-in metal, and the oracle has nothing else.  The device
gets it through debug_set_spectra, and what it must return follows from the term itself: with all-zero spectra the term is -1 in every bin
wherever c^2 > 0 and NaN where c^2 = 0, so value = (fd * 1 + (-1) * 0) * term has the bits the oracle gives with any metal, or is NaN in
all 16 bins; and the pdf does not depend on the spectra.  On the rows made to have c = 0 the value IS NaN -- the unflagged pair ran the
term -- where the same material with its built-in metal gives a number.

Render parity: a 96 x 64 frame of a cube on a floor -- Uber faces with metalness_mul = 0 (flagged pair), 0.5, and 0 on the unflagged pair,
Lambert faces and floor, a sun and a sky -- at depth 8, 24 launches, accumulator and result image against the oracle as uint32, in both
launch modes; then the first face goes to metalness_mul = 0.5 through update_materials_and_lights, 8 more launches, compared again.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import glaze_amd
from glaze_amd import abi
from glaze_amd.scene_desc import INSTANCE_DTYPE, MESH_DTYPE, make_camera, make_light, make_material, make_meta
from glaze_amd.scenes import cube_scene
from oracle.pyoracle import OracleRenderer, OracleScene
from test_gpu_shading_routines import SAMPLE_FIELDS, VALUE_FIELDS, assert_call_equal, same_bits, sphere_dirs

N = 384
GOLD, GERMANIUM, SILVER = 2, 13, 0
TEX_METALNESS, TEX_SKY = 2, 3
UV_TEXEL_0, UV_TEXEL_255 = (0.25, 0.5), (0.75, 0.5)     # the centres of the 2 x 1 metalness map's texels
BELOW_HALF = np.nextafter(np.float32(0.5), np.float32(0.0))
# material ids (0 .. 2 are cube_scene's)
FLAGGED, UNFLAGGED, HALF, MAPPED, ZEROED = 3, 4, 5, 6, 7


def materials():
    common = dict(mtype=abi.MAT_UBER, roughness_mul=0.6, anisotropy=0.3, ior=1.5, diffuse_mul=(200, 150, 100))
    return [make_material("flagged, metalness 0", metal=GOLD, metalness_mul=0.0, **common),
            make_material("unflagged, metalness 0", metal=GERMANIUM, metalness_mul=0.0, **common),
            make_material("metalness 0.5", metal=GOLD, metalness_mul=0.5, **common),
            make_material("metalness map", metal=GOLD, metalness_mul=1.0, metalness=TEX_METALNESS, **common),
            make_material("for the all-zero pair", metal=SILVER, metalness_mul=0.0, **common)]


def sky_pixels():
    rng = np.random.default_rng(7)
    tex = rng.integers(1, 256, (12, 24, 4), dtype=np.uint8)
    tex[..., 3] = 255
    return tex


@functools.lru_cache(maxsize=None)
def call_desc():
    desc = cube_scene()
    desc.textures += [(abi.TEX_GRAY, np.array([[0, 255]], np.uint8), "metalness")]
    assert len(desc.textures) == TEX_METALNESS + 1
    desc.materials += materials()
    assert len(desc.materials) == ZEROED + 1
    return desc


@functools.lru_cache(maxsize=None)
def oracle_scene():
    return OracleScene(call_desc())


@pytest.fixture(scope="module")
def gpu_scene(instance):
    return glaze_amd.RayTraceScene.from_desc(instance, call_desc())


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------
C0_ROWS = slice(0, 32)          # wi = (wo.x, wo.y, -wo.z): both normalise by the same length, wh.z = 0 exactly, c = 0
HORIZON_ROWS = slice(32, 40)    # wo.z = wi.z = 0
BACK_ROWS = slice(40, 72)       # wi = -wo: wh = normalize(0) is NaN
MIRROR_ROWS = slice(72, 104)    # wi = (-wo.x, -wo.y, wo.z): wh is the normal, c = |wo.z|


@functools.lru_cache(maxsize=None)
def value_inputs():
    rng = np.random.default_rng(11)
    wo, wi = sphere_dirs(N, rng), sphere_dirs(N, rng)
    same_side = np.arange(N) % 3 != 0                                                  # two rows in three reflect: the lobe is zero across the surface
    wi[same_side, 2] = np.copysign(wi[same_side, 2], wo[same_side, 2])
    wi[C0_ROWS] = wo[C0_ROWS] * np.array([1, 1, -1], np.float32)
    phi = rng.uniform(0.0, 2.0 * np.pi, (2, 8))
    wo[HORIZON_ROWS] = np.stack([np.cos(phi[0]), np.sin(phi[0]), np.zeros(8)], -1).astype(np.float32)
    wi[HORIZON_ROWS] = np.stack([np.cos(phi[1]), np.sin(phi[1]), np.zeros(8)], -1).astype(np.float32)
    wi[BACK_ROWS] = -wo[BACK_ROWS]
    wi[MIRROR_ROWS] = wo[MIRROR_ROWS] * np.array([-1, -1, 1], np.float32)
    r1 = rng.random(N, dtype=np.float32)
    r1[:104] = np.resize(np.array([0.1, 0.4, BELOW_HALF, 0.0], np.float32), 104)     # the made rows take the specular lobe ...
    r1[104::8] = 0.5                                                                    # ... the others both, and the split itself
    r1[105::8] = BELOW_HALF
    assert (wo[:, 2] > 0).sum() > N // 4 and (wo[:, 2] < 0).sum() > N // 4
    assert (r1 < 0.5).sum() > N // 3 and (r1 >= 0.5).sum() > N // 4
    for a in (wo, wi, r1):
        a.setflags(write=False)
    return wo, wi, r1


@functools.lru_cache(maxsize=None)
def sample_inputs():
    rng = np.random.default_rng(12)
    wo = sphere_dirs(N, rng)
    wo[:8] = [(0, 0, 1), (0, 0, -1), (1, 0, 0), (0, -1, 0), (0.6, 0, 0.8), (0.6, 0, -0.8), (1, 0, 1e-7), (1, 0, -1e-7)]
    r3 = rng.random((N, 3), dtype=np.float32)
    r3[0::8, 2] = 0.5
    r3[1::8, 2] = BELOW_HALF
    r3[2::16, 0] = 0.0
    r3[3::16, 1] = np.float32(0.99999994)
    assert (wo[:, 2] > 0).sum() > N // 4 and (wo[:, 2] < 0).sum() > N // 4
    assert (r3[:, 2] < 0.5).sum() > N // 3 and (r3[:, 2] >= 0.5).sum() > N // 3
    wo.setflags(write=False)
    r3.setflags(write=False)
    return wo, r3


CASES = (("flagged pair, metalness 0", FLAGGED, (0.5, 0.5)), ("unflagged pair, metalness 0", UNFLAGGED, (0.5, 0.5)),
         ("metalness 0.5", HALF, (0.5, 0.5)), ("metalness map, texel 0", MAPPED, UV_TEXEL_0), ("metalness map, texel 255", MAPPED, UV_TEXEL_255),
         ("silver, metalness 0", ZEROED, (0.5, 0.5)))
IDS = [c[0] for c in CASES]


def value_of(side, case):
    wo, wi, r1 = value_inputs()
    fn = side.bsdf_value if isinstance(side, OracleScene) else side.debug_bsdf_value
    return fn(case[1], wo, wi, uv=case[2], rand=r1)


def sample_of(side, case):
    wo, r3 = sample_inputs()
    fn = side.bsdf_sample if isinstance(side, OracleScene) else side.debug_bsdf_sample
    return fn(case[1], wo, r3, uv=case[2])


@functools.lru_cache(maxsize=None)
def oracle_value(case):
    return value_of(oracle_scene(), case)


@functools.lru_cache(maxsize=None)
def oracle_sample(case):
    return sample_of(oracle_scene(), case)


# ---------------------------------------------------------------------------------------------------------------------
# without a device: the cases are what they say
# ---------------------------------------------------------------------------------------------------------------------
def test_the_cases_are_what_they_say():
    def flag(metal):
        n, a, out = np.zeros(16, np.float32), np.zeros(16, np.float32), C.c_int(-1)
        abi.check(abi.lib().glz_host_metal_spectra(metal, n.ctypes.data, a.ctypes.data))
        abi.check(abi.lib().glz_host_conductor_finite(n.ctypes.data, a.ctypes.data, C.byref(out)))
        return out.value

    assert flag(GOLD) == 1 and flag(SILVER) == 1 and flag(GERMANIUM) == 0
    # the map's two texels give a metalness of exactly 0 and exactly 1
    tex = oracle_scene().sample_texture(TEX_METALNESS, [UV_TEXEL_0, UV_TEXEL_255])
    assert tex[0, 0] == 0.0 and tex[1, 0] == 1.0
    # the conductor term shows in the oracle's values where the metalness is not zero, and nowhere else: with metalness 0 gold, germanium and
    # silver give the same bits, and the map's black texel the same as metalness_mul = 0
    by_name = {c[0]: oracle_value(c) for c in CASES}
    zero = by_name["flagged pair, metalness 0"]
    for name in ("unflagged pair, metalness 0", "silver, metalness 0", "metalness map, texel 0"):
        assert same_bits(by_name[name][0], zero[0]).all() and same_bits(by_name[name][1], zero[1]).all(), name
    live = zero[1] > 0
    assert live.sum() > N // 4
    for name in ("metalness 0.5", "metalness map, texel 255"):
        assert same_bits(by_name[name][1], zero[1]).all()
        assert (~same_bits(by_name[name][0], zero[0]).all(-1) & live).sum() > N // 8, name
    for c in CASES:
        wi, value, pdf = oracle_sample(c)
        assert not np.isnan(pdf).any() and (pdf > 0).sum() > N // 4, c[0]
    # the made rows: a NaN half vector and a half vector in the surface end with a pdf of 0 (NaN -> 0 by check_nan; wo.z wi.z <= 0)
    assert (zero[1][BACK_ROWS] == 0).all() and (zero[1][C0_ROWS] == 0).all()
    assert (zero[1][MIRROR_ROWS] > 0).any()


# ---------------------------------------------------------------------------------------------------------------------
# device against oracle, call by call
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_bsdf_value_equals_oracle(gpu_scene, case):
    wo, wi, r1 = value_inputs()
    assert_call_equal("bsdf_value, " + case[0], value_of(gpu_scene, case), oracle_value(case), VALUE_FIELDS, {"wo": wo, "wi": wi, "rand": r1})


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_bsdf_sample_equals_oracle(gpu_scene, case):
    wo, r3 = sample_inputs()
    assert_call_equal("bsdf_sample, " + case[0], sample_of(gpu_scene, case), oracle_sample(case), SAMPLE_FIELDS, {"wo": wo, "rand3": r3})


@pytest.mark.gpu
def test_all_zero_spectra_run_the_term(instance, gpu_scene):
    case = CASES[-1]
    zeroed = glaze_amd.RayTraceScene.from_desc(instance, call_desc())
    zeroed.debug_set_spectra(ZEROED, np.zeros(16, np.float32), np.zeros(16, np.float32))
    with pytest.raises(abi.GlazeError):
        zeroed.debug_set_spectra(ZEROED + 1, np.zeros(16, np.float32), np.zeros(16, np.float32))
    wo, wi, r1 = value_inputs()
    specular = r1 < 0.5

    def value_or_nan(got, want):
        return same_bits(got, want).all(-1) | np.isnan(got).all(-1)

    # bsdf_value: against the oracle (its silver) by the rule, the value also allowed to be NaN in all bins; against the device's own silver
    # on every row, dead ones included
    value_z, pdf_z = value_of(zeroed, case)
    value_o, pdf_o = oracle_value(case)
    value_s, pdf_s = value_of(gpu_scene, case)
    assert same_bits(pdf_z, pdf_o).all() and same_bits(pdf_z, pdf_s).all()
    assert value_or_nan(value_z, value_o)[pdf_o > 0].all()
    assert value_or_nan(value_z, value_s).all()
    assert same_bits(value_z, value_s)[~specular].all()                       # the diffuse lobe has no conductor term
    # c = 0: NaN with the all-zero pair, a number with silver, whose flag let the lane skip the term (and whose term is finite there)
    for rows in (C0_ROWS, HORIZON_ROWS):
        assert specular[rows].all()
    assert np.isnan(value_z[C0_ROWS]).all()
    assert np.isfinite(value_s[C0_ROWS]).all()
    # off c = 0 the term is -1, times 0: most rows keep silver's bits
    assert same_bits(value_z, value_s).all(-1).mean() > 0.8
    # bsdf_sample: the same two comparisons
    wi_z, sv_z, sp_z = sample_of(zeroed, case)
    wi_o, sv_o, sp_o = oracle_sample(case)
    wi_s, sv_s, sp_s = sample_of(gpu_scene, case)
    assert same_bits(sp_z, sp_o).all() and same_bits(sp_z, sp_s).all()
    assert same_bits(wi_z, wi_s).all()
    assert same_bits(wi_z, wi_o)[sp_o > 0].all()
    assert value_or_nan(sv_z, sv_o)[sp_o > 0].all()
    assert value_or_nan(sv_z, sv_s).all()
    assert same_bits(sv_z, sv_s).all(-1).mean() > 0.8
    # the other materials of the scene are untouched by the hook
    flagged = CASES[0]
    assert_call_equal("bsdf_value next to the all-zero pair", value_of(zeroed, flagged), oracle_value(flagged), VALUE_FIELDS, {"wo": wo, "wi": wi, "rand": r1})


# ---------------------------------------------------------------------------------------------------------------------
# render parity
# ---------------------------------------------------------------------------------------------------------------------
SIZE, DEPTH, LAUNCHES, LAUNCHES_AFTER = (96, 64), 8, 24, 8
MODES = ("two_kernels", "path")
TOP, FRONT, LEFT, BOTTOM, RIGHT, BACK = range(6)     # the cube's faces in index order, by their normals: +y, +z, -x, -y, +x, -z


@functools.lru_cache(maxsize=None)
def box_desc(after_update=False):
    """the cube seen from outside (the specular lobe is zero on a face hit from behind), three of its faces Uber and two Lambert, on a Lambert
    floor -- the top face's mesh again, four times as wide and two units down, where the cube's own bottom would be -- under a sun and a sky"""
    desc = cube_scene()
    desc.textures += [(abi.TEX_GRAY, np.array([[0, 255]], np.uint8), "metalness"), (abi.TEX_RGBA_SRGB, sky_pixels(), "sky")]
    assert len(desc.textures) == TEX_SKY + 1
    common = dict(mtype=abi.MAT_UBER, roughness_mul=0.5, ior=1.5, diffuse=1)
    first = len(desc.materials)
    desc.materials += [make_material("wall, metalness 0", metal=GOLD, metalness_mul=0.5 if after_update else 0.0, diffuse_mul=(230, 200, 180), **common),
                       make_material("wall, metalness 0.5", metal=GOLD, metalness_mul=0.5, diffuse_mul=(180, 240, 190), **common),
                       make_material("wall, unflagged pair", metal=GERMANIUM, metalness_mul=0.0, diffuse_mul=(200, 220, 240), **common),
                       make_material("lambert", diffuse=1, diffuse_mul=(220, 220, 220))]
    uber0, uber_half, uber_ge, lambert = range(first, first + 4)
    faces = ((FRONT, uber0), (RIGHT, uber_ge), (TOP, uber_half), (LEFT, lambert), (BACK, lambert), (TOP, lambert))
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
def oracle_images(after_update, launches):
    o = OracleRenderer(OracleScene(box_desc(after_update)), *SIZE)
    o.set_depth(DEPTH)
    o.set_seed(3)
    o.step(launches)
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


def test_the_update_shows_in_the_oracle_image():
    before, after = oracle_images(False, LAUNCHES_AFTER), oracle_images(True, LAUNCHES_AFTER)
    assert (before[1][..., :3] != 0).any() and not np.array_equal(before[1], after[1])


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_render_keeps_every_bit_before_and_after_a_material_update(instance, mode):
    r = glaze_amd.RayTraceRenderer.new(instance, glaze_amd.RayTraceScene.from_desc(instance, box_desc()), *SIZE)
    r.set_launch_mode(mode)
    r.set_depth(DEPTH)
    r.set_seed(3)
    r.step(LAUNCHES)
    assert r.launch_mode() == mode
    assert_same(r, oracle_images(False, LAUNCHES), "%s, %d launches" % (mode, LAUNCHES))
    cur = box_desc(True)
    r.update_materials_and_lights(cur.materials, cur.lights)
    r.step(LAUNCHES_AFTER)
    assert_same(r, oracle_images(True, LAUNCHES_AFTER), "%s, %d launches after the update" % (mode, LAUNCHES_AFTER))
