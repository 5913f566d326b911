"""Any-hit rays walk the hierarchy farthest child first (GLZ_ANY_FAR_FIRST, device/trace_wave.h); closest-hit rays keep nearest first.

An occluded ray is occluded whichever occluder is found first and an unoccluded ray visits the same nodes in any order, so nothing a
tracer reports may change: occlusion is compared with the oracle element for element (1), and whole renders bit for bit (2) -- in both
launch modes (k_trace's pass of shadow rays only, k_path's mixed pass with the order chosen per lane) and over both node widths.
"""
import numpy as np
import pytest

import glaze_amd
from glaze_amd import abi
from glaze_amd.scene_desc import INSTANCE_DTYPE, make_light
from glaze_amd.scenes import atrium_scene, cube_scene
from oracle.pyoracle import OracleRenderer, OracleScene

from conftest import MATTEST
from helpers import desc_from_oracle_parse

pytestmark = pytest.mark.gpu

N_RAYS = 20_000
SUN = np.array([0.35, 0.85, -0.25]) / np.linalg.norm([0.35, 0.85, -0.25])


def bits(a):
    return np.nan_to_num(a, nan=-1.0).view(np.uint32)


def small_atrium():
    return atrium_scene(detail=0.05, texture_size=64, sky_size=(256, 128))


def instanced_cubes(n, seed):
    """the cube mesh n times under random rotations, non-uniform scales and mirrors, inside the cube itself as the room"""
    rng = np.random.default_rng(seed)
    d = cube_scene(material_type=abi.MAT_UBER)
    mats = [np.eye(4)]
    for _ in range(n):
        a, b, c = rng.uniform(0, 2 * np.pi, 3)
        rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
        ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
        rz = np.array([[np.cos(c), -np.sin(c), 0], [np.sin(c), np.cos(c), 0], [0, 0, 1]])
        m = np.eye(4)
        m[:3, :3] = rx @ ry @ rz @ np.diag(rng.uniform(0.02, 0.12, 3) * np.where(rng.random(3) < 0.15, -1.0, 1.0))
        m[:3, 3] = rng.uniform(-0.8, 0.8, 3)
        mats.append(m)
    d.transforms = np.stack([np.asarray(m, np.float32).T.reshape(16) for m in mats])
    d.instances = np.array([(0, i) for i in range(len(mats))], INSTANCE_DTYPE)
    d.lights.append(make_light(abi.LIGHT_SUN, "sun", direction=(0.2, -0.7, 0.4), intensity=0.5))
    return d


def world_bounds(desc):
    """bounds of the instanced geometry, from the description alone"""
    lo, hi = np.full(3, np.inf), np.full(3, -np.inf)
    for inst in desc.instances:
        mesh = desc.meshes[int(inst["mesh_id"])]
        idx = desc.indices[int(mesh["index_offset"]): int(mesh["index_offset"]) + int(mesh["index_count"])]
        p = desc.vertices["vv"][np.unique(idx)].astype(np.float64)
        m = desc.transforms[int(inst["transform_id"])].reshape(4, 4).T.astype(np.float64)
        w = p @ m[:3, :3].T + m[:3, 3]
        lo, hi = np.minimum(lo, w.min(0)), np.maximum(hi, w.max(0))
    return lo, hi


def unit(d):
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


def shadow_like_rays(desc, orc, seed):
    """N_RAYS rays of the kinds a render traces as shadow rays, and the degenerate ones:
      * 8 000 from random points inside the bounds in random directions;
      * 6 000 + 6 000 from surfaces -- the closest hits of the first set, o + t d as k_shade stores the point (it does not move the origin
        off the surface: the shadow ray's tmin, 1e-3, does that) -- towards one fixed sun direction and towards random directions of the
        upper hemisphere;
      * slab-parallel rays, rays along an edge and a zero direction (test_axis_aligned_and_degenerate_rays).
    tmax: every second ray infinite, the others uniform in (0, 3)."""
    rng = np.random.default_rng(seed)
    lo, hi = world_bounds(desc)
    n_a, n_b = 8000, 6000
    o_a = (lo + rng.random((n_a, 3)) * (hi - lo)).astype(np.float32)
    d_a = unit(rng.normal(size=(n_a, 3)))
    t, tri, _, _, _ = orc.trace_closest(o_a, d_a)
    hit = np.flatnonzero(np.isfinite(t) & (tri != 0xFFFFFFFF))
    assert hit.size > 1000
    pick = hit[rng.integers(0, hit.size, 2 * n_b)]
    p = (o_a[pick] + d_a[pick] * t[pick, None]).astype(np.float32)
    d_sun = np.broadcast_to(SUN.astype(np.float32), (n_b, 3))
    d_sky = rng.normal(size=(n_b, 3))
    d_sky[:, 1] = np.abs(d_sky[:, 1])
    o_deg = np.array([[0, 0, 0]] * 6 + [[1, 1, 0], [0.999999, 0.999999, 0], [0, 0, 0], [0, 0, 0]], np.float32)
    d_deg = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [0, 0, 1], [0, 0, 1], [0, 0, 0], [1, 1, 1]], np.float32)
    o = np.concatenate([o_a, p, o_deg])
    d = np.concatenate([d_a, d_sun, unit(d_sky), d_deg]).astype(np.float32)
    tmax = rng.uniform(0.0, 3.0, o.shape[0]).astype(np.float32)
    tmax[::2] = np.inf
    assert o.shape[0] == N_RAYS + 10
    return o, d, tmax


SCENES = {
    "cube": lambda: cube_scene(),
    "mattest": lambda: desc_from_oracle_parse(MATTEST),
    "atrium": small_atrium,
    "instances_flat": lambda: instanced_cubes(60, seed=4),
    "instances_two_level": lambda: instanced_cubes(60, seed=4),
}


@pytest.mark.parametrize("which", list(SCENES))
def test_any_hit_parity(instance, which):
    desc = SCENES[which]()
    if which == "mattest":
        gpu = glaze_amd.RayTraceScene.new(instance, glaze_amd.parse(MATTEST))      # the product's reader, as the product loads it
    else:
        levels = {"instances_flat": "flat", "instances_two_level": "two_level"}.get(which, "auto")
        instance.set_as_levels(levels)
        try:
            gpu = glaze_amd.RayTraceScene.from_desc(instance, desc)
        finally:
            instance.set_as_levels("auto")
        if levels != "auto":
            assert gpu.info().as_levels == (1 if levels == "flat" else 2)
    orc = OracleScene(desc)
    o, d, tmax = shadow_like_rays(desc, orc, seed=11)
    want = orc.trace_any(o, d, tmax)
    got = gpu.debug_trace_any(o, d, tmax)
    print("%s: occluded %.3f of %d rays" % (which, want.mean(), want.size))
    assert 0.05 < want.mean() < 0.95            # neither all-miss nor all-hit
    assert np.array_equal(got, want), "rays that differ: %s" % np.flatnonzero(got != want)[:20]


def render_pair(instance, desc, w, h, depth, seed, mode, node_width):
    r = glaze_amd.RayTraceRenderer.new(instance, glaze_amd.RayTraceScene.from_desc(instance, desc), w, h)
    r.set_launch_mode(mode)
    if node_width:
        r.set_node_width(node_width)
        assert r.node_width() == node_width
    r.set_depth(depth)
    r.set_seed(seed)
    return r


@pytest.fixture(scope="module")
def atrium_reference():
    desc = small_atrium()
    o = OracleRenderer(OracleScene(desc), 96, 64)
    o.set_depth(6)
    o.set_seed(7)
    o.step(12)
    return desc, o.read_hdr()


@pytest.mark.parametrize("mode,node_width", [("two_kernels", 4), ("two_kernels", 8), ("path", 4), ("path", 8)])
def test_render_parity_small_atrium(instance, atrium_reference, mode, node_width):
    desc, want = atrium_reference
    r = render_pair(instance, desc, 96, 64, 6, 7, mode, node_width)
    r.step(12)
    got = r.read_hdr()
    assert np.array_equal(bits(got), bits(want)), "%d pixels differ" % (bits(got) != bits(want)).any(-1).sum()
    assert (got[..., :3].sum(-1) > 0).mean() > 0.5


def test_render_parity_small_atrium_with_opacity_maps(instance):
    """k_trace<kAlphaPhase>, and its shadow pass on its own: a read between two runs of launches drains the queued shadow rays in a
    launch that traces nothing else"""
    desc = atrium_scene(sponza_like=True, texture_size=64, sky_size=(64, 32))
    o = OracleRenderer(OracleScene(desc), 150, 83)
    o.set_depth(6)
    o.set_seed(7)
    o.step(24)
    want = o.read_hdr()
    a = render_pair(instance, desc, 150, 83, 6, 7, "two_kernels", 0)
    b = render_pair(instance, desc, 150, 83, 6, 7, "two_kernels", 0)
    a.step(24)
    b.step(7)
    b.read_hdr()
    b.step(17)
    assert np.array_equal(bits(a.read_hdr()), bits(b.read_hdr()))
    assert np.array_equal(bits(a.read_hdr()), bits(want)), "%d pixels differ" % (bits(a.read_hdr()) != bits(want)).any(-1).sum()
