"""Through-specular guides (glz_renderer_set_guide_mode, GLZ_GUIDE_THROUGH_SPECULAR): the feature buffers of the first non-specular vertex
along the ray the path itself follows through Mirror and Glass.

The chain's rays must equal the oracle's path bit for bit (its state after launch L is the ray the path traces from its L-th vertex: the
first launch's pixel offset is the pixel centre); the planes must equal what the oracle's closest hits of those rays imply; the default
mode must not change in any bit; nothing may disturb a running accumulation.
"""
import os
import subprocess

import numpy as np
import pytest
from PIL import Image

import glaze_amd
from glaze_amd import abi
from glaze_amd.scene_desc import make_camera
from glaze_amd.scenes import MIRROR_ROOM_PLANE_Z, cube_scene, forest_scene, mirror_room_scene
from oracle.pyoracle import OracleRenderer, OracleScene, launch_constants

from conftest import MATTEST
from helpers import camera_rays, desc_from_oracle_parse
from test_gpu_denoise import bits, restate_first_hit, small_atrium

pytestmark = pytest.mark.gpu

CLI = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "glaze_amd", "csrc", "glaze-cli")
W, H = 128, 72
BSDF_MIRROR, BSDF_GLASS = 6, 8           # RTMaterial::bsdf_index (device/types.h)
MISS = np.uint32(0xFFFFFFFF)


def new_renderer(instance, desc, levels="auto", size=(W, H)):
    instance.set_as_levels(levels)
    try:
        scene = glaze_amd.RayTraceScene.from_desc(instance, desc)
    finally:
        instance.set_as_levels("auto")
    if levels == "two_level":
        assert scene.info().as_levels == 2
    if levels == "flat":
        assert scene.info().as_levels == 1
    return glaze_amd.RayTraceRenderer.new(instance, scene, size[0], size[1])


def planes(ren):
    return ren.read_aov("normal_depth"), ren.read_aov("albedo_instance")


def material_tables(desc, orc):
    """per RTMaterial: bsdf_index, is_specular; per instance: its material"""
    raw = orc.rt_materials().reshape(-1, 208)
    bsdf = raw[:, 180:184].copy().view(np.uint32)[:, 0]
    specular = raw[:, 200:204].copy().view(np.uint32)[:, 0] != 0
    meshes = {int(m["id"]): m for m in desc.meshes}
    inst_material = np.array([int(meshes[int(i["mesh_id"])]["material"]) for i in desc.instances], np.int64)
    assert (specular == ((bsdf == BSDF_MIRROR) | (bsdf == BSDF_GLASS))).all()
    return bsdf, specular, inst_material


class Chain:
    """One scene under test: its description, the oracle's scene and a renderer, made once for the tests that share them."""

    def __init__(self, instance, desc, levels):
        self.desc, self.orc = desc, OracleScene(desc)
        self.ren = new_renderer(instance, desc, levels)
        self.bsdf, self.specular, self.inst_material = material_tables(desc, self.orc)

    def hook(self, segment):
        o, d, alive = self.ren.debug_guide_chain(segment)
        return o.reshape(-1, 3), d.reshape(-1, 3), alive.reshape(-1)

    def material_of(self, hit, inst):
        return self.inst_material[np.where(hit, inst, 0).astype(np.int64)]


CHAIN_SCENES = {"mattest": (lambda: desc_from_oracle_parse(MATTEST), "auto"), "room_flat": (mirror_room_scene, "flat"),
                "room_two_level": (mirror_room_scene, "two_level"), "facing": (lambda: mirror_room_scene(view="facing"), "flat")}
_chains = {}


@pytest.fixture
def chain(instance, request):
    name = request.param
    if name not in _chains:
        make, levels = CHAIN_SCENES[name]
        _chains[name] = Chain(instance, make(), levels)
    return name, _chains[name]


# ---------------------------------------------------------------------------------------------------------------------
# 1. the default is untouched
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cube", "forest", "atrium"])
def test_scenes_without_specular_materials_give_the_same_planes_in_both_modes(instance, name):
    make, levels = {"cube": (cube_scene, "auto"), "forest": (lambda: forest_scene(40), "two_level"), "atrium": (small_atrium, "auto")}[name]
    desc = make()
    untouched = planes(new_renderer(instance, desc, levels))
    ren = new_renderer(instance, desc, levels)
    assert ren.guide_mode()[0] == "first_hit"
    first = planes(ren)
    ren.set_guide_mode("through_specular", 3)
    assert ren.guide_mode() == ("through_specular", 3)
    through = planes(ren)
    for k in (1, 2, 3, 4):                                            # no chain has a second segment
        assert not ren.debug_guide_chain(k)[2].any()
    assert ren.debug_guide_chain(0)[2].all()
    for bad in ((2, 4), (-1, 4), ("through_specular", 0), ("through_specular", 9), ("through_specular", 0xFFFFFFFF)):
        with pytest.raises(glaze_amd.GlazeError) as e:
            ren.set_guide_mode(*bad)
        assert e.value.status == abi.E_ARG
        assert ren.guide_mode() == ("through_specular", 3)
    ren.set_guide_mode("first_hit", 0)                               # max_bounces is ignored in first-hit mode
    assert ren.guide_mode()[0] == "first_hit"
    again = planes(ren)
    assert np.isfinite(first[0][..., 3]).any()
    for a, b, c, d in zip(untouched, first, through, again):
        assert np.array_equal(bits(a), bits(b)) and np.array_equal(bits(a), bits(c)) and np.array_equal(bits(a), bits(d))


# ---------------------------------------------------------------------------------------------------------------------
# 2. the chain's rays are the oracle's path, bit for bit
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chain", ["mattest", "room_flat", "room_two_level"], indirect=True)
def test_chain_rays_equal_the_oracle_path(instance, chain):
    name, c = chain
    B = 4
    c.ren.set_guide_mode("through_specular", B)
    assert launch_constants(1, 0)[1] == (0.5, 0.5)                    # the first launch goes through the pixel centres
    orc_ren = OracleRenderer(c.orc, W, H)
    orc_ren.set_seed(1)
    orc_ren.set_depth(16)                                             # no roulette within eight bounces
    o, d, alive = c.hook(0)
    assert alive.all()
    ho, hd = camera_rays(c.ren.push_constants(), W, H)
    assert np.abs(o - ho).max() <= 1e-6 * max(1.0, np.abs(ho).max()) and np.abs(d - hd).max() <= 1e-6
    compared = np.ones(W * H, bool)
    counts = []
    for L in range(1, B + 1):
        orc_ren.step(1)
        state = orc_ren.read_state().reshape(-1, 24)
        wi, flag, point, bounce = state[:, 16:19], state[:, 19], state[:, 20:23], state[:, 23]
        idx = np.flatnonzero(compared)
        t, tri, inst, u, v = c.orc.trace_closest(o[idx], d[idx], tmin=1e-4)
        hit = np.isfinite(t)
        _, normal, _, _, _ = restate_first_hit(c.desc, c.orc, o[idx], d[idx], t, tri, inst, u, v)
        material = c.material_of(hit, inst)
        specular = hit & c.specular[material]
        mirror, glass = specular & (c.bsdf[material] == BSDF_MIRROR), specular & (c.bsdf[material] == BSDF_GLASS)
        with np.errstate(all="ignore"):
            cos_in = (d[idx].astype(np.float64) * normal).sum(-1)
            cos_out = (wi[idx].astype(np.float64) * normal).sum(-1)
        clear = (np.abs(cos_in) > 1e-3) & (np.abs(cos_out) > 1e-3)
        transmitted = glass & clear & (cos_in * cos_out > 0)           # the next direction lies on the other side of the surface
        reflected = glass & clear & (cos_in * cos_out < 0)
        unclear = glass & ~clear
        follow = mirror | transmitted
        counts.append((int(follow.sum()), int(reflected.sum()), int(unclear.sum())))
        assert unclear.sum() == 0
        compared = np.zeros(W * H, bool)
        compared[idx[follow]] = True
        assert (bounce[compared] == L).all() and (flag[compared] == 1).all()   # the oracle's path is at its L-th vertex, on a specular one
        o, d, alive = c.hook(L)
        assert alive[compared].all()
        differ = (bits(o[compared]) != bits(point[compared])).any(-1) | (bits(d[compared]) != bits(wi[compared])).any(-1)
        assert not differ.any(), "segment %d: %d of %d rays differ from the oracle's state, first at pixel %d" % (
            L, differ.sum(), compared.sum(), np.flatnonzero(compared)[np.argmax(differ)])
        if L == 1 and name.startswith("room"):                        # every pixel on the large mirror is compared
            on_mirror = np.zeros(W * H, bool)
            on_mirror[idx[hit & (inst == len(c.desc.instances) - 1)]] = True
            assert on_mirror.sum() * 3 >= W * H and compared[on_mirror].all()
    print("%s: (compared, oracle reflected, unclear) at vertices 1 .. %d: %s" % (name, B, counts))
    if name == "mattest":
        assert counts[0][0] >= 4000 and counts[1][0] >= 2000
        # the oracle needs a scene description, which its own reader made; the library's reader (parse) must lead to the same chain
        parsed = glaze_amd.RayTraceRenderer.new(instance, glaze_amd.RayTraceScene.new(instance, glaze_amd.parse(MATTEST)), W, H)
        parsed.set_guide_mode("through_specular", B)
        for L in range(B + 2):
            for got, want in zip(parsed.debug_guide_chain(L), c.ren.debug_guide_chain(L)):
                assert np.array_equal(bits(got) if got.dtype == np.float32 else got, bits(want) if want.dtype == np.float32 else want)
        for got, want in zip(planes(parsed), planes(c.ren)):
            assert np.array_equal(bits(got), bits(want))
    else:
        assert counts[0][0] >= 3000 and counts[1][0] >= 1000


# ---------------------------------------------------------------------------------------------------------------------
# 3. hits and planes along the chain
# ---------------------------------------------------------------------------------------------------------------------
def walk_chain(c, B):
    """The hook's rays of every segment through the oracle's tracer: what the specification makes of the hits (the reporting vertex's
    depth, instance, albedo, normal), with the hook's `alive` checked on the way.  Returns per-pixel arrays."""
    n = W * H
    f = np.float32
    out = dict(depth=np.full(n, np.inf, f), inst=np.full(n, MISS, np.uint32), albedo=np.ones((n, 3), f), normal=np.zeros((n, 3)), dir=np.zeros((n, 3), f),
               mapped=np.zeros(n, bool), vertex=np.full(n, -1), capped=np.zeros(n, bool))
    running = np.zeros(n, f)
    expect_alive = np.ones(n, bool)
    for k in range(B + 1):
        o, d, alive = c.hook(k)
        assert np.array_equal(alive, expect_alive), "segment %d: alive differs at %d pixels" % (k, (alive != expect_alive).sum())
        assert (o[~alive] == 0).all() and (d[~alive] == 0).all()
        idx = np.flatnonzero(alive)
        expect_alive = np.zeros(n, bool)
        if idx.size == 0:
            continue
        t, tri, inst, u, v = c.orc.trace_closest(o[idx], d[idx], tmin=1e-4)
        hit = np.isfinite(t)
        albedo, normal, _, mapped, _ = restate_first_hit(c.desc, c.orc, o[idx], d[idx], t, tri, inst, u, v)
        at = idx[hit]
        running[at] = t[hit] if k == 0 else running[at] + t[hit]      # ((t0 + t1) + ...) + tk in binary32
        out["depth"][at], out["inst"][at], out["albedo"][at], out["normal"][at] = running[at], inst[hit], albedo[hit], normal[hit]
        out["dir"][at], out["mapped"][at], out["vertex"][at] = d[idx][hit], mapped[hit], k
        specular = hit & c.specular[c.material_of(hit, inst)]
        if k < B:
            expect_alive[idx[specular]] = True
        else:
            out["capped"][idx[specular]] = True                       # vertex B is specular: the cap ends the chain
    assert not c.hook(B + 1)[2].any()
    return out


def check_planes(c, B, want):
    nd, ai = (p.reshape(-1, 4) for p in planes(c.ren))
    assert np.array_equal(bits(nd[:, 3]), bits(want["depth"])), "%d depths differ" % (bits(nd[:, 3]) != bits(want["depth"])).sum()
    assert np.array_equal(bits(ai[:, 3]), want["inst"]), "%d instances differ" % (bits(ai[:, 3]) != want["inst"]).sum()
    differ = (bits(ai[:, :3]) != bits(want["albedo"])).any(-1)
    assert not differ.any(), "%d albedo values differ, first at %s" % (differ.sum(), np.flatnonzero(differ)[0])
    hit = want["vertex"] >= 0
    assert (nd[~hit, :3] == 0).all()
    err = np.abs(nd[:, :3].astype(np.float64) - want["normal"]).max(-1)
    plain, mapped = hit & ~want["mapped"], hit & want["mapped"]
    print("  B = %d: reporting vertices %s, %d ended by the cap, normal max abs err %.3g plain, %.3g mapped" % (
        B, np.bincount(want["vertex"][hit]).tolist(), want["capped"].sum(), err[plain].max() if plain.any() else 0.0, err[mapped].max() if mapped.any() else 0.0))
    assert not plain.any() or err[plain].max() <= 1e-5
    assert not mapped.any() or err[mapped].max() <= 2e-5
    assert np.abs(np.linalg.norm(nd[hit, :3].astype(np.float64), axis=-1) - 1.0).max() <= 1e-5
    assert ((nd[hit, :3].astype(np.float64) * want["dir"][hit]).sum(-1) <= 0).all()


@pytest.mark.parametrize("chain", ["mattest", "room_flat", "room_two_level"], indirect=True)
def test_planes_follow_the_oracle_hits_along_the_chain(chain):
    name, c = chain
    B = 4
    c.ren.set_guide_mode("through_specular", B)
    want = walk_chain(c, B)
    print(name)
    check_planes(c, B, want)
    assert (want["vertex"] >= 1).sum() >= 3000                        # the chains are there
    # a pixel whose first hit is not specular has the same bits in both modes
    c.ren.set_guide_mode("first_hit")
    first = [p.reshape(-1, 4) for p in planes(c.ren)]
    c.ren.set_guide_mode("through_specular", B)
    o, d, _ = c.hook(0)
    t, tri, inst, u, v = c.orc.trace_closest(o, d, tmin=1e-4)
    direct = ~(np.isfinite(t) & c.specular[c.material_of(np.isfinite(t), inst)])
    assert direct.sum() >= 1000 and (~direct).sum() >= 3000
    for got, ref in zip((p.reshape(-1, 4) for p in planes(c.ren)), first):
        assert np.array_equal(bits(got[direct]), bits(ref[direct]))
    assert (bits(planes(c.ren)[0].reshape(-1, 4)[~direct, 3]) != bits(first[0][~direct, 3])).sum() >= 3000   # and the others have moved on


@pytest.mark.parametrize("chain", ["facing"], indirect=True)
@pytest.mark.parametrize("B", [1, 2, 4, 8])
def test_the_cap_ends_the_chain_between_facing_mirrors(chain, B):
    name, c = chain
    c.ren.set_guide_mode("through_specular", B)
    want = walk_chain(c, B)
    check_planes(c, B, want)
    assert want["capped"].sum() >= 300
    assert (want["vertex"][want["capped"]] == B).all()                # the reporting vertex is the B-th reflection
    assert (c.bsdf[c.inst_material[want["inst"][want["capped"]]]] == BSDF_MIRROR).all()


# ---------------------------------------------------------------------------------------------------------------------
# 4. a planar mirror is a virtual camera
# ---------------------------------------------------------------------------------------------------------------------
# measured on an MI355X (see the docstring below): gate = the next power of ten above, and never above 1e-4
MEASURED_DEPTH_REL, MEASURED_NORMAL_ABS, MEASURED_ALBEDO_ABS = 3.98e-7, 1.19e-7, 2.14e-5
GATE_DEPTH_REL, GATE_NORMAL_ABS, GATE_ALBEDO_ABS = 1e-6, 1e-6, 1e-4


def virtual_camera_errors(instance):
    desc = mirror_room_scene()
    ren = new_renderer(instance, desc, "flat")
    ren.set_guide_mode("through_specular", 1)                         # vertex 1 reports whatever it is, as a first hit does
    nd, ai = planes(ren)
    ren.set_guide_mode("first_hit")
    on_mirror = bits(ren.read_aov(1)[..., 3]) == len(desc.instances) - 1
    assert on_mirror.sum() * 3 >= W * H

    def reflected(v, w):                                              # in the plane z = MIRROR_ROOM_PLANE_Z (w = 0: a direction)
        return (v[0], v[1], 2.0 * MIRROR_ROOM_PLANE_Z * w - v[2])

    cam = desc.camera
    behind = mirror_room_scene(mirror=False)
    behind.camera = make_camera(position=reflected(cam.position, 1), target=reflected(cam.target, 1), up=reflected(cam.up, 0), fovx=cam.fovx_or_scale,
                                near=cam.near_plane, far=cam.far_plane)
    vnd, vai = (p[:, ::-1] for p in planes(new_renderer(instance, behind, "flat")))   # a reflection flips the image left-right
    same = on_mirror & (bits(ai[..., 3]) == bits(vai[..., 3]))
    excluded = (on_mirror & ~same).sum() / on_mirror.sum()
    hit = same & np.isfinite(vnd[..., 3])
    assert hit.sum() >= 0.9 * on_mirror.sum()
    assert np.array_equal(np.isfinite(nd[..., 3])[same], np.isfinite(vnd[..., 3])[same])
    depth = np.abs(nd[..., 3][hit].astype(np.float64) - vnd[..., 3][hit]) / vnd[..., 3][hit]
    # (the reflected camera looks at the room itself, not at its mirror image: its ray IS the chain's second segment unfolded, so the two
    # normals are the same world-space vector, turned against the same direction -- nothing is reflected back)
    normal = np.abs(nd[..., :3][hit].astype(np.float64) - vnd[..., :3][hit])
    albedo = np.abs(ai[..., :3][hit].astype(np.float64) - vai[..., :3][hit])
    return excluded, depth.max(), normal.max(), albedo.max()


def test_a_planar_mirror_is_a_virtual_camera(instance):
    """Through-specular planes (cap 1) of the pixels whose first hit is the large mirror against the first-hit planes of the room without
    that mirror from the camera reflected in its plane.  The share of pixels left out for an instance mismatch (silhouettes) is a
    condition: at most 0.5 % (the oracle alone, a float64 reflection of the centre rays against the reflected camera: 0 of 3 963).

    Measured (MI355X, 128 x 72): no pixel excluded; depth 3.98e-7 relative, normal 1.19e-7, albedo 2.14e-5 absolute -> gates 1e-6, 1e-6,
    1e-4 (with 128-texel, full-contrast checkers the albedo differed by 1.2e-4: the two hit points differ in their last bits and a bilinear
    texel edge magnifies that, which is why the room's textures have 32 texels)."""
    excluded, depth, normal, albedo = virtual_camera_errors(instance)
    print("virtual camera: excluded %.4f %%, depth rel %.3g, normal abs %.3g, albedo abs %.3g" % (100 * excluded, depth, normal, albedo))
    assert excluded <= 0.005
    assert depth <= GATE_DEPTH_REL and normal <= GATE_NORMAL_ABS and albedo <= GATE_ALBEDO_ABS


# ---------------------------------------------------------------------------------------------------------------------
# 5. it helps the denoiser where it should
# ---------------------------------------------------------------------------------------------------------------------
SEEDS = (1, 2, 3, 4, 5, 6, 7, 8)
# measured on an MI355X with the default parameters and cap 4, seeds 1 .. 8 (see the docstring of the test)
MEASURED = (0.9113, 0.9025, 0.9090, 0.9567, 0.9639, 0.9604, 0.9195, 0.9302)
GATE = (max(MEASURED) * 1.0) ** 0.5                    # 0.9818: halfway, in log terms, between the worst seed and no improvement


def guide_ratios(instance):
    """per seed: MSE(denoised with through-specular guides, converged) / MSE(denoised with first-hit guides, converged) over the pixels whose
    first hit is the large mirror, without the 1 % of them whose NOISY error is largest"""
    size = (256, 144)
    desc = mirror_room_scene()
    ren = new_renderer(instance, desc, "auto", size)
    ren.set_depth(8)
    ren.set_seed(987654321)
    ren.draw(512, want_image=False)
    converged = ren.read_result()[..., :3].astype(np.float64)
    on_mirror = bits(ren.read_aov(1)[..., 3]) == len(desc.instances) - 1
    ratios = []
    for seed in SEEDS:
        ren = new_renderer(instance, desc, "auto", size)
        ren.set_depth(8)
        ren.set_seed(seed)
        ren.draw(2, want_image=False)
        noisy = ren.read_result()[..., :3].astype(np.float64)
        first = ren.read_denoised()[..., :3].astype(np.float64)
        ren.set_guide_mode("through_specular", 4)
        through = ren.read_denoised()[..., :3].astype(np.float64)
        ok = on_mirror & np.isfinite(noisy).all(-1) & np.isfinite(first).all(-1) & np.isfinite(through).all(-1) & np.isfinite(converged).all(-1)
        e_noisy = ((noisy - converged) ** 2).sum(-1)
        keep = ok & (e_noisy <= np.quantile(e_noisy[ok], 0.99))
        ratios.append(((through - converged) ** 2).sum(-1)[keep].mean() / ((first - converged) ** 2).sum(-1)[keep].mean())
    return ratios


def dilated(mask, radius):
    """the pixels within `radius` (Chebyshev) of a pixel of `mask`"""
    out = mask.copy()
    for axis in (0, 1):
        src = out.copy()
        for shift in range(1, radius + 1):
            lo, hi = [slice(None)] * 2, [slice(None)] * 2
            lo[axis], hi[axis] = slice(shift, None), slice(None, -shift)
            out[tuple(hi)] |= src[tuple(lo)]
            out[tuple(lo)] |= src[tuple(hi)]
    return out


def test_through_specular_guides_help_inside_the_mirror(instance):
    """mirror_room_scene() at 256 x 144, depth 8, 2 spp against 512 spp of the unfiltered path with another seed, over the pixels whose first
    hit is the large mirror without the 1 % whose noisy error is largest: MSE(denoised with through-specular guides) / MSE(denoised with
    first-hit guides) must be below 1, and below the gate: the geometric mean of the worst measured seed's ratio and 1.

    Measured (MI355X, default parameters, cap 4), seeds 1 .. 8: 0.9113, 0.9025, 0.9090, 0.9567, 0.9639, 0.9604, 0.9195, 0.9302 -> gate
    0.9818.  The scene matters more than the guides: with a glass slab made by scaling the cube to 4 % (the shading normal is not
    renormalised after the inverse-transpose, so every bounce off it multiplies the path's weight by 25) the 2-spp image and the 512-spp
    one were both fields of fireflies of 1e5 times the median radiance, the MSE was theirs alone, and the ratios came out between 0.80 and
    5.7: whichever filter spread a firefly further won.  Every transform of the room is now a similarity."""
    ratios = guide_ratios(instance)
    print("MSE ratios (through-specular / first-hit guides) inside the mirror over seeds %s: %s" % (SEEDS, ", ".join("%.4f" % r for r in ratios)))
    assert max(ratios) < 1.0
    assert max(ratios) < GATE


@pytest.mark.parametrize("iterations", [5, 2])
def test_denoised_pixels_out_of_reach_of_specular_ones_do_not_change(instance, iterations):
    """A pixel whose first hit is not specular has the same guides in both modes, but its filtered value also reads its neighbours': pass k
    reaches 2 * 2^k pixels, `iterations` passes 2 (2^iterations - 1).  Out of that reach of every pixel whose planes differ between the
    modes the two denoised images are bit-identical (with five passes, 62 pixels, few pixels of this frame qualify; with two, most of
    the non-specular ones do)."""
    desc = mirror_room_scene()
    ren = new_renderer(instance, desc, "auto", (256, 144))
    ren.set_depth(8)
    ren.set_seed(1)
    ren.draw(2, want_image=False)
    ren.set_denoise(iterations=iterations)
    first_planes, first = planes(ren), ren.read_denoised()
    ren.set_guide_mode("through_specular", 4)
    through_planes, through = planes(ren), ren.read_denoised()
    moved = (bits(first_planes[0]) != bits(through_planes[0])).any(-1) | (bits(first_planes[1]) != bits(through_planes[1])).any(-1)
    assert moved.sum() >= 256 * 144 // 3
    far = ~dilated(moved, 2 * (2 ** iterations - 1))
    changed = (bits(first) != bits(through)).any(-1)
    print("iterations %d: %d pixels moved their guides, %d out of their reach, %d denoised pixels changed" % (iterations, moved.sum(), far.sum(), changed.sum()))
    assert not changed[far].any()
    assert changed[moved].sum() >= moved.sum() // 2                    # where the guides moved the filter follows them
    if iterations == 2:
        assert far.sum() >= 5000


# ---------------------------------------------------------------------------------------------------------------------
# 6. nothing else moves
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("config", ["two_kernels", "path", "chains3"])
def test_guide_reads_do_not_disturb_the_accumulation(instance, config):
    desc = mirror_room_scene()

    def renderer():
        r = new_renderer(instance, desc, "auto", (150, 83))
        r.set_seed(21)
        r.set_depth(4)
        if config == "chains3":
            r.set_chains(3)
        else:
            r.set_launch_mode(config)
        return r

    a, b = renderer(), renderer()
    a.step(24)
    b.step(7)
    b.set_guide_mode("through_specular", 4)
    nd, ai = planes(b)
    den = b.read_denoised()
    assert np.array_equal(bits(den), bits(glaze_amd.host_denoise(b.read_result(), nd, ai)))
    b.set_guide_mode("first_hit")
    assert (bits(planes(b)[0]) != bits(nd)).any(-1).sum() >= 3000    # the mode did something in between
    b.set_guide_mode("through_specular", 2)
    b.read_denoised()
    b.step(17)
    assert np.array_equal(bits(a.read_hdr()), bits(b.read_hdr()))
    assert np.array_equal(bits(a.read_result()), bits(b.read_result()))
    assert a.stats().launches == b.stats().launches == 24


# ---------------------------------------------------------------------------------------------------------------------
# 7. CLI
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists(CLI), reason="glaze-cli is not built")
def test_cli_guides_writes_what_the_library_returns(tmp_path, instance):
    png, prefix = str(tmp_path / "o.png"), str(tmp_path / "aov")
    r = subprocess.run([CLI, MATTEST, png, "-r", "96x64", "-s", "1", "--guides", "through-specular:2", "--aov-out", prefix], capture_output=True, text=True)
    assert r.returncode == 0 and "All done :)" in r.stderr, r.stderr
    ren = glaze_amd.RayTraceRenderer.new(instance, glaze_amd.RayTraceScene.new(instance, glaze_amd.parse(MATTEST)), 96, 64)
    first = ren.read_aov(0)
    ren.set_guide_mode("through_specular", 2)
    nd, ai = planes(ren)
    assert (bits(first[..., 3]) != bits(nd[..., 3])).sum() >= 1000
    assert np.array_equal(np.fromfile(prefix + ".depth.bin", "<f4").view(np.uint32), bits(nd[..., 3]).ravel())
    normal_png = np.asarray(Image.open(prefix + ".normal.png"))[..., :3]
    assert np.abs(normal_png.astype(np.float64) - (nd[..., :3] * 0.5 + 0.5) * 255.0).max() <= 0.5 + 1e-3
    albedo = ai.copy()
    albedo[..., 3] = 1.0
    tm = np.zeros((64, 96, 4), np.uint8)
    abi.check(abi.lib().glz_debug_tonemap(instance._h, np.ascontiguousarray(albedo).ctypes.data, 96 * 64, tm.ctypes.data))
    assert np.array_equal(np.asarray(Image.open(prefix + ".albedo.png"))[..., :3], tm[..., :3])
    for bad in ("through-specular:0", "through-specular:9", "through-specular:", "mirrors"):
        r = subprocess.run([CLI, MATTEST, png, "--guides", bad], capture_output=True, text=True)
        assert r.returncode == 2 and "--guides" in r.stderr
