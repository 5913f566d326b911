"""Moving instances under a live renderer (glz_renderer_update_transforms).

Closest hits do not depend on the shape of the tree (ties on t go to the smaller world triangle id), and a rebuilt structure is
built by the same code from the same inputs, so the rule is strict: a scene A created with transforms T0 and updated to T1 must be
indistinguishable from a scene B created fresh with T1 -- node for node, record for record, hit for hit and pixel for pixel.  A
flattened scene is rebuilt in full; a two-level scene keeps its meshes' hierarchies and rebuilds the top level over instance boxes
that a device kernel computes bit for bit as the host rule does.
"""
import numpy as np
import pytest

import glaze_amd
from glaze_amd import abi
from glaze_amd.scene_desc import INSTANCE_DTYPE, MESH_DTYPE, make_light, make_material
from glaze_amd.scenes import cube_scene, forest_scene
from oracle.pyoracle import OracleRenderer, OracleScene

pytestmark = pytest.mark.gpu


def bits(a):
    return np.nan_to_num(np.asarray(a, np.float32), nan=-1.0).view(np.uint32)


def col_major(m):
    return np.asarray(m, np.float32).T.reshape(16)


def random_transforms(rng, n, scale=(0.02, 0.12), spread=0.8):
    """rotations, non-uniform scales, mirrors and a few identities"""
    out = []
    for i in range(n):
        if i % 9 == 4:
            out.append(col_major(np.eye(4)))
            continue
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        m = np.eye(4)
        m[:3, :3] = q @ np.diag(rng.uniform(scale[0], scale[1], 3) * np.where(rng.random(3) < 0.15, -1.0, 1.0))
        m[:3, 3] = rng.uniform(-spread, spread, 3)
        out.append(col_major(m))
    return np.stack(out)


def instanced_cubes(n, seed=0, emissive_every=0, opacity=False):
    """the room (transform 0, the identity) and n small cubes; every `emissive_every`-th cube is an area light (the same index range
    as a second mesh with an emissive material: the two-level build shares one hierarchy)"""
    rng = np.random.default_rng(seed)
    d = cube_scene(material_type=abi.MAT_UBER)
    d.transforms = np.concatenate([col_major(np.eye(4))[None], random_transforms(rng, n)])
    mesh_of = [0] + [1 if emissive_every and i % emissive_every == 0 else 0 for i in range(n)]
    d.meshes = np.array([(0, 2, 0, 36), (1, 3, 0, 36)], MESH_DTYPE)
    d.materials.append(make_material("lamp", emissive=(255, 230, 200)))
    d.instances = np.array([(m, i) for i, m in enumerate(mesh_of)], INSTANCE_DTYPE)
    d.lights.append(make_light(abi.LIGHT_SUN, "sun", direction=(0.2, -0.7, 0.4), intensity=0.5))
    if emissive_every:
        d.lights.append(make_light(abi.LIGHT_AREA, "lamps", resource_id=3, intensity=3.0))
    if opacity:
        y, x = np.mgrid[0:64, 0:64]
        d.textures.append((abi.TEX_GRAY, np.where(((x // 8 + y // 8) % 2) == 0, 255, 0).astype(np.uint8), "alpha"))
        d.materials[2].opacity = 2
    return d


def with_transforms(desc, t):
    d = desc.copy()
    d.transforms = np.ascontiguousarray(t, np.float32).reshape(-1, 16)
    return d


def make_scene(instance, desc, levels, builder="auto"):
    instance.set_as_levels(levels)
    instance.set_bvh_builder(builder)
    try:
        return glaze_amd.RayTraceScene.from_desc(instance, desc)
    finally:
        instance.set_as_levels("auto")
        instance.set_bvh_builder("auto")


def info_fields(scene):
    """glz_scene_info but for build_ms and the SAH cost, which the builders sum with float atomics (reported only, order not fixed)"""
    i = scene.info()
    return {name: (list(getattr(i, name)) if hasattr(getattr(i, name), "__len__") else getattr(i, name))
            for name, _ in i._fields_ if name not in ("build_ms", "bvh_sah_cost")}


def assert_same_structure(a, b):
    assert info_fields(a) == info_fields(b)
    assert a.info().bvh_sah_cost == pytest.approx(b.info().bvh_sah_cost, rel=1e-5, nan_ok=True)
    na, ta = a.debug_bvh()
    nb, tb = b.debug_bvh()
    assert np.array_equal(na, nb) and np.array_equal(bits(ta), bits(tb))
    assert np.array_equal(a.debug_bvh8(), b.debug_bvh8())
    assert np.array_equal(a.debug_tlas_instances(), b.debug_tlas_instances())
    assert np.array_equal(a.debug_rt_lights(), b.debug_rt_lights())


def assert_boxes_match_host(scene, budgets=(0,)):
    """the device kernel against the host rule, bit for bit (two-level scenes)"""
    for budget in budgets:
        dev = scene.debug_instance_boxes(True, budget)
        host = scene.debug_instance_boxes(False, budget)
        assert dev is not None and host is not None
        for x, y in zip(dev, host):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), budget


def random_rays(info, n, seed=0):
    rng = np.random.default_rng(seed)
    lo, hi = np.array(info.bounds_min, np.float64), np.array(info.bounds_max, np.float64)
    lo, hi = np.where(np.isfinite(lo), lo, -10.0), np.where(np.isfinite(hi), hi, 10.0)
    c, ext = 0.5 * (lo + hi), np.maximum(hi - lo, 1e-3)
    o = (c + rng.uniform(-0.6, 0.6, (n, 3)) * ext).astype(np.float32)
    d = rng.normal(size=(n, 3))
    axis = rng.random(n) < 0.15                                                                # axis-parallel rays
    k = rng.integers(0, 3, n)
    d[axis] = 0.0
    d[axis, k[axis]] = np.where(rng.random(axis.sum()) < 0.5, -1.0, 1.0)
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    tmax = (rng.uniform(0.0, 1.0, n) * np.linalg.norm(ext)).astype(np.float32)
    return o, d, tmax


def assert_same_hits(a, b, n=200_000, seed=0):
    o, d, tmax = random_rays(b.info(), n, seed)
    ha, hb = a.debug_trace_closest(o, d), b.debug_trace_closest(o, d)
    for x, y in zip(ha, hb):
        assert np.array_equal(bits(x) if x.dtype == np.float32 else x, bits(y) if y.dtype == np.float32 else y)
    assert np.isfinite(ha[0]).any()                                                             # the rays do hit something
    assert np.array_equal(a.debug_trace_any(o, d, tmax), b.debug_trace_any(o, d, tmax))


def render(r, k, seed=3, depth=4, mode="auto", chains=0):
    r.set_launch_mode(mode)
    r.set_chains(chains)
    r.set_depth(depth)
    r.set_seed(seed)
    r.step(k)
    return r.read_hdr(), r.read_result()


def assert_same_render(ra, rb, **kw):
    for x, y in zip(render(ra, 5, **kw), render(rb, 5, **kw)):
        assert np.array_equal(bits(x), bits(y)), kw


def check_update(instance, desc, t1, levels, builder="auto", rays=200_000, size=(64, 48), **render_kw):
    """A (T0, then updated to T1) against B (created with T1): structure, hits, renders; returns (A, B, A's renderer)"""
    a = make_scene(instance, desc, levels, builder)
    ra = glaze_amd.RayTraceRenderer.new(instance, a, *size)
    ra.update_transforms(t1)
    b = make_scene(instance, with_transforms(desc, t1), levels, builder)
    assert a.info().as_levels == b.info().as_levels == {"flat": 1, "two_level": 2}.get(levels, b.info().as_levels)
    assert_same_structure(a, b)
    if b.info().as_levels == 2:
        assert a.debug_box_kernel_ms() >= 0.0                                                   # the update ran the box kernels
        assert_boxes_match_host(a)
    if rays:
        assert_same_hits(a, b, rays)
    rb = glaze_amd.RayTraceRenderer.new(instance, b, *size)
    assert_same_render(ra, rb, **render_kw)
    return a, b, ra


# ---- 1-3: structure, hits, renders ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("levels", ["flat", "two_level"])
@pytest.mark.parametrize("builder", ["sah", "lbvh", "ploc"])
def test_updated_instanced_cubes_equal_a_fresh_scene(instance, levels, builder):
    desc = instanced_cubes(150, seed=1)
    t1 = desc.transforms.copy()
    t1[1:] = random_transforms(np.random.default_rng(2), 150)
    check_update(instance, desc, t1, levels, builder, rays=200_000 if builder == "sah" else 50_000)


@pytest.mark.parametrize("levels", ["flat", "two_level"])
def test_updated_forest_equals_a_fresh_scene(instance, levels):
    desc = forest_scene(300)
    rng = np.random.default_rng(4)
    t1 = desc.transforms.copy().reshape(-1, 4, 4)
    t1[1:, 3, 0] += rng.uniform(-3, 3, 300).astype(np.float32)                                  # move the columns (row 3 = translation)
    t1[1:, 3, 2] += rng.uniform(-3, 3, 300).astype(np.float32)
    t1[1::5, 0, 0] *= np.float32(-1.0)                                                          # and mirror some
    check_update(instance, desc, t1.reshape(-1, 16), levels)


@pytest.mark.parametrize("mode,chains", [("two_kernels", 1), ("two_kernels", 3), ("path", 1), ("path", 3)])
def test_renders_match_in_every_launch_mode_and_chain_count(instance, mode, chains):
    desc = instanced_cubes(40, seed=6, emissive_every=5)
    t1 = desc.transforms.copy()
    t1[1:] = random_transforms(np.random.default_rng(7), 40)
    for levels in ("flat", "two_level"):
        a = make_scene(instance, desc, levels)
        ra = glaze_amd.RayTraceRenderer.new(instance, a, 136, 72)
        ra.update_transforms(t1)
        rb = glaze_amd.RayTraceRenderer.new(instance, make_scene(instance, with_transforms(desc, t1), levels), 136, 72)
        assert_same_render(ra, rb, mode=mode, chains=chains)


@pytest.mark.parametrize("levels", ["flat", "two_level"])
def test_updated_render_matches_the_oracle(instance, levels):
    desc = instanced_cubes(12, seed=8, emissive_every=4)
    t1 = desc.transforms.copy()
    t1[1:] = random_transforms(np.random.default_rng(9), 12)
    a = make_scene(instance, desc, levels)
    r = glaze_amd.RayTraceRenderer.new(instance, a, 48, 32)
    r.update_transforms(t1)
    img, _ = render(r, 5, seed=7, depth=4)
    o = OracleRenderer(OracleScene(with_transforms(desc, t1)), 48, 32)
    o.set_depth(4)
    o.set_seed(7)
    o.step(5)
    assert np.array_equal(bits(img), bits(o.read_hdr()))


# ---- 4: round trip, restart ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("levels", ["flat", "two_level"])
def test_round_trip_gives_back_the_original_scene(instance, levels):
    desc = instanced_cubes(60, seed=10, emissive_every=7)
    t0 = desc.transforms.copy()
    t1 = t0.copy()
    t1[1:] = random_transforms(np.random.default_rng(11), 60, spread=0.3)
    a = make_scene(instance, desc, levels)
    before_nodes, before_tris = a.debug_bvh()
    before_recs = a.debug_tlas_instances()
    ra = glaze_amd.RayTraceRenderer.new(instance, a, 64, 48)
    first = render(ra, 5)
    ra.update_transforms(t1)
    moved = render(ra, 5)
    assert not np.array_equal(bits(first[0]), bits(moved[0]))
    ra.update_transforms(t0)
    nodes, tris = a.debug_bvh()
    assert np.array_equal(nodes, before_nodes) and np.array_equal(bits(tris), bits(before_tris))
    assert np.array_equal(a.debug_tlas_instances(), before_recs)
    again = render(ra, 5)
    for x, y in zip(first, again):
        assert np.array_equal(bits(x), bits(y))


def test_an_update_mid_render_restarts_accumulation(instance):
    desc = instanced_cubes(30, seed=12)
    t1 = desc.transforms.copy()
    t1[1:] = random_transforms(np.random.default_rng(13), 30)
    for levels in ("flat", "two_level"):
        a = make_scene(instance, desc, levels)
        ra = glaze_amd.RayTraceRenderer.new(instance, a, 64, 48)
        ra.set_depth(4)
        ra.set_seed(3)
        ra.step(7)                                                                               # mid-render
        ra.update_transforms(t1)
        ra.step(5)
        rb = glaze_amd.RayTraceRenderer.new(instance, make_scene(instance, with_transforms(desc, t1), levels), 64, 48)
        rb.set_depth(4)
        rb.set_seed(3)
        rb.step(5)
        assert ra.read_hdr()[..., 3].max() == 5                                                  # five launches since the update
        assert np.array_equal(bits(ra.read_hdr()), bits(rb.read_hdr()))
        assert np.array_equal(bits(ra.read_result()), bits(rb.read_result()))


# ---- 5: hard cases -------------------------------------------------------------------------------------------------------------
def hard_transforms(desc, rng):
    t = desc.transforms.copy()
    n = t.shape[0] - 1
    t[1:] = random_transforms(rng, n)
    mirror = np.eye(4)
    mirror[:3, :3] = np.diag([-0.05, 0.07, 0.06])
    mirror[:3, 3] = (0.3, -0.2, 0.5)
    t[1] = col_major(mirror)                                                                   # negative determinant
    t[2] = 0.0                                                                                 # zero scale (singular)
    t[2][15] = 1.0
    t[3] = np.nan                                                                              # NaN
    t[4] = col_major(np.eye(4))
    t[4][12] = np.inf                                                                          # an infinite translation
    t[5] = col_major(np.eye(4))
    t[5][[1, 2, 3, 4, 6, 7, 8, 9, 11, 12, 13, 14]] = -0.0                                       # the identity with -0.0 entries
    return t


@pytest.mark.parametrize("levels", ["flat", "two_level"])
def test_hard_transforms_area_lights_and_opacity_maps(instance, levels):
    desc = instanced_cubes(50, seed=14, emissive_every=3, opacity=True)
    t1 = hard_transforms(desc, np.random.default_rng(15))
    a, b, _ = check_update(instance, desc, t1, levels, rays=100_000, depth=6)
    if levels == "two_level":
        assert a.debug_tlas_instances().size == 192 * desc.instances.shape[0]


def test_clustering_deepens_the_top_level_and_the_traversal_stack(instance):
    """every instance moved into one geometric cluster: the SAH top level gets much deeper than a spread-out one, past what the
    traversal keeps in LDS, and the renderer's spill area grows with it"""
    n = 64
    desc = instanced_cubes(n, seed=16)
    t1 = desc.transforms.copy()
    for i in range(n):
        m = np.eye(4)
        m[:3, :3] *= 0.01
        m[:3, 3] = (0.5 - 0.7 * 0.8 ** i, 0.1 * 0.8 ** i, 0.3)
        t1[1 + i] = col_major(m)
    a, b, ra = check_update(instance, desc, t1, "two_level", rays=50_000)
    before = make_scene(instance, desc, "two_level").info().bvh_depth
    after = a.info().bvh_depth
    assert after > before and 3 * after + 2 > 17, (before, after)                              # kTraversalLdsStack = 17 entries in LDS


# ---- 6: several devices --------------------------------------------------------------------------------------------------------
@pytest.fixture
def loopback(monkeypatch):
    monkeypatch.setenv("GLAZE_MULTI_LOOPBACK", "1")


@pytest.mark.parametrize("levels", ["flat", "two_level"])
def test_loopback_devices_follow_an_update(instance, loopback, levels):
    desc = instanced_cubes(40, seed=17, emissive_every=5)
    t1 = desc.transforms.copy()
    t1[1:] = random_transforms(np.random.default_rng(18), 40)
    r = glaze_amd.RayTraceRenderer.new(instance, make_scene(instance, desc, levels), 136, 200)
    r.set_devices([instance.device] * 3)
    r.update_transforms(t1)
    one = glaze_amd.RayTraceRenderer.new(instance, make_scene(instance, with_transforms(desc, t1), levels), 136, 200)
    assert_same_render(r, one)
    assert np.array_equal(r.read_rgba8(), one.read_rgba8())


# ---- 7: the box kernel against the host rule -----------------------------------------------------------------------------------
def test_box_kernel_equals_the_host_rule_with_and_without_the_corner_fallback(instance):
    cubes = instanced_cubes(80, seed=19, emissive_every=3)
    cubes = with_transforms(cubes, hard_transforms(cubes, np.random.default_rng(20)))
    for desc, budget in ((cubes, 24 * 30), (forest_scene(200), 3_000 * 50)):                 # ~30 cubes / ~50 columns exact
        a = make_scene(instance, desc, "two_level")
        assert_boxes_match_host(a, (0, budget))
        exact = a.debug_instance_boxes(False)
        lo, hi = a.debug_instance_boxes(False, budget)
        same = (lo.view(np.uint32) == exact[0].view(np.uint32)).all(1) & (hi.view(np.uint32) == exact[1].view(np.uint32)).all(1)
        assert same[:10].all() and not same.all()                                              # the fallback starts partway through


# ---- 8: errors -----------------------------------------------------------------------------------------------------------------
def test_bad_arguments_change_nothing(instance):
    desc = instanced_cubes(20, seed=21)
    for levels in ("flat", "two_level"):
        r = glaze_amd.RayTraceRenderer.new(instance, make_scene(instance, desc, levels), 64, 48)
        ref = glaze_amd.RayTraceRenderer.new(instance, make_scene(instance, desc, levels), 64, 48)
        for x in (r, ref):
            x.set_depth(4)
            x.set_seed(5)
            x.step(3)
        with pytest.raises(glaze_amd.GlazeError) as e:
            r.update_transforms(desc.transforms[:-1])
        assert e.value.status == abi.E_ARG
        assert abi.lib().glz_renderer_update_transforms(r._h, None, desc.transforms.shape[0]) == abi.E_ARG
        with pytest.raises(ValueError):
            r.update_transforms(desc.transforms.reshape(-1, 4, 4))
        for x in (r, ref):
            x.step(4)
        assert np.array_equal(bits(r.read_hdr()), bits(ref.read_hdr()))
        assert np.array_equal(bits(r.read_result()), bits(ref.read_result()))
