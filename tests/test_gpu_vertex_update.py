"""Deforming meshes under a live renderer (glz_renderer_update_vertices).

The rule is the one of test_gpu_transform_update.py: a scene A created with vertices V0 and updated to V1 must give, hit for hit and
pixel for pixel, what a scene B created fresh with V1 gives -- closest hits do not depend on the shape of the tree, so the refitted
hierarchy of A and the freshly built one of B are two witnesses of the same scene.  Where the vertices do not change (an identity
update, a round trip) the refit must also reproduce the builder's bytes: that is the exactness test of the fit and quantise kernels.

Launch modes: the renderers know 'auto', 'two_kernels' and 'path', and a chain count; "where they apply" here means the flattened scenes
(k_path and the 8-wide nodes exist for those alone).
"""
import numpy as np
import pytest

import glaze_amd
from glaze_amd import abi
from glaze_amd.scene_desc import INSTANCE_DTYPE, MESH_DTYPE, VERTEX_DTYPE, make_light, make_material
from glaze_amd.scenes import cube_scene
from oracle.pyoracle import OracleRenderer, OracleScene

pytestmark = pytest.mark.gpu

HAS_PARTNER, QUAD_SWAPPED = 0x40000000, 0x20000000


# ---- helpers (after test_gpu_transform_update.py) ------------------------------------------------------------------------------
def bits(a):
    return np.nan_to_num(np.asarray(a, np.float32), nan=-1.0).view(np.uint32)


def col_major(m):
    return np.asarray(m, np.float32).T.reshape(16)


def random_transforms(rng, n, scale=(0.1, 0.3), spread=0.6):
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


def make_scene(instance, desc, levels="flat", builder="auto"):
    instance.set_as_levels(levels)
    instance.set_bvh_builder(builder)
    try:
        return glaze_amd.RayTraceScene.from_desc(instance, desc)
    finally:
        instance.set_as_levels("auto")
        instance.set_bvh_builder("auto")


def info_fields(scene, but=("build_ms", "bvh_sah_cost")):
    i = scene.info()
    return {name: (list(getattr(i, name)) if hasattr(getattr(i, name), "__len__") else getattr(i, name)) for name, _ in i._fields_ if name not in but}


def structure(scene):
    """every byte of the structure a tracer reads, and the info that describes it"""
    nodes, tris = scene.debug_bvh()
    return dict(nodes=nodes, tris=bits(tris), nodes8=scene.debug_bvh8(), leaves=scene.debug_leaf_records(), top=scene.debug_tlas_instances(),
                info=info_fields(scene))


def assert_same_bytes(x, y, but=()):
    for key in x:
        if key in but:
            continue
        assert x[key] == y[key] if key == "info" else np.array_equal(x[key], y[key]), key


def assert_same_structure(a, b):
    """test_gpu_transform_update.py's rule for two structures the same builder made of the same inputs"""
    assert info_fields(a) == info_fields(b)
    assert a.info().bvh_sah_cost == pytest.approx(b.info().bvh_sah_cost, rel=1e-5, nan_ok=True)
    assert_same_bytes(structure(a), structure(b))
    assert np.array_equal(a.debug_rt_lights(), b.debug_rt_lights())


def random_rays(info, n, seed=0):
    rng = np.random.default_rng(seed)
    lo, hi = np.array(info.bounds_min, np.float64), np.array(info.bounds_max, np.float64)
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


def render(r, k=5, seed=3, depth=4, mode="auto", chains=0, width=0):
    r.set_launch_mode(mode)
    r.set_node_width(width)
    r.set_chains(chains)
    r.set_depth(depth)
    r.set_seed(seed)
    r.step(k)
    return r.read_hdr(), r.read_result()


def assert_same_render(ra, rb, **kw):
    for x, y in zip(render(ra, **kw), render(rb, **kw)):
        assert np.array_equal(bits(x), bits(y)), kw


def assert_same_bounds_and_grid(a, b):
    ia, ib = a.info(), b.info()
    for name in ("bounds_min", "bounds_max", "bvh_grid_lo", "bvh_grid_cell"):
        assert np.array_equal(bits(list(getattr(ia, name))), bits(list(getattr(ib, name)))), name


def tris_by_world_id(scene):
    """the triangle records in world-triangle order, without the bit that says how the builder grouped them into leaves"""
    t = bits(scene.debug_bvh()[1]).copy()
    t[:, 11] &= ~np.uint32(HAS_PARTNER)
    return t[np.argsort(t[:, 3], kind="stable")]


# ---- scenes --------------------------------------------------------------------------------------------------------------------
N_ROOM = 24   # vertices of cube_scene's room: the sheet's follow


def sheet(n=32, y=-0.4, x=(-0.7, 0.7), z=(0.2, 0.9)):
    """(n + 1)^2 vertices and 2 n^2 triangles in fan order: each cell is (a, b, c), (a, c, d), the order a quad leaf takes as it is"""
    s, t = np.meshgrid(np.linspace(0, 1, n + 1, dtype=np.float32), np.linspace(0, 1, n + 1, dtype=np.float32), indexing="ij")
    v = np.zeros((n + 1) * (n + 1), VERTEX_DTYPE)
    v["vv"] = np.stack([x[0] + s * (x[1] - x[0]), np.full_like(s, y), z[0] + t * (z[1] - z[0])], -1).reshape(-1, 3)
    v["vn"] = (0.0, 1.0, 0.0)
    v["vt"] = np.stack([s, t], -1).reshape(-1, 2)
    idx = np.arange((n + 1) * (n + 1), dtype=np.uint32).reshape(n + 1, n + 1)
    a, b, c, d = idx[:-1, :-1], idx[:-1, 1:], idx[1:, 1:], idx[1:, :-1]
    return v, np.stack([a, b, c, a, c, d], -1).reshape(-1)


def sheet_scene(n=32, opacity=False, emissive=False, room=True):
    """the 33 x 33-vertex sheet (2 048 triangles, more than 256 leaves) inside cube_scene's room, or alone"""
    d = cube_scene(material_type=abi.MAT_UBER)
    v, idx = sheet(n)
    d.materials.append(make_material("sheet", mtype=abi.MAT_UBER, diffuse_mul=(230, 200, 170), diffuse=1, emissive=(255, 220, 180) if emissive else None))
    if room:
        d.vertices = np.concatenate([d.vertices, v])
        d.indices = np.concatenate([d.indices, idx + np.uint32(N_ROOM)])
        d.meshes = np.array([(0, 2, 0, 36), (1, 3, 36, idx.size)], MESH_DTYPE)
        d.instances = np.array([(0, 0), (1, 0)], INSTANCE_DTYPE)
    else:
        d.vertices, d.indices = v, idx
        d.meshes = np.array([(0, 3, 0, idx.size)], MESH_DTYPE)
        d.instances = np.array([(0, 0)], INSTANCE_DTYPE)
    d.lights.append(make_light(abi.LIGHT_SUN, "sun", direction=(0.2, -0.7, 0.4), intensity=0.5))
    if emissive:
        d.lights.append(make_light(abi.LIGHT_AREA, "sheet", resource_id=3, intensity=3.0))
    if opacity:
        y, x = np.mgrid[0:64, 0:64]
        d.textures.append((abi.TEX_GRAY, np.where(((x // 8 + y // 8) % 2) == 0, 255, 0).astype(np.uint8), "alpha"))
        d.materials[3].opacity = 2
    return d


def waved(vertices, amp=0.15, phase=0.0, first=N_ROOM):
    """a sine wave across the sheet: positions and normals"""
    v = vertices.copy()
    p = v["vv"][first:].astype(np.float64)
    kx, kz = 9.0, 7.0
    p[:, 1] += amp * np.sin(kx * p[:, 0] + phase) * np.cos(kz * p[:, 2])
    n = np.stack([-amp * kx * np.cos(kx * p[:, 0] + phase) * np.cos(kz * p[:, 2]), np.ones(len(p)), amp * kz * np.sin(kx * p[:, 0] + phase) * np.sin(kz * p[:, 2])], -1)
    v["vv"][first:] = p.astype(np.float32)
    v["vn"][first:] = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(np.float32)
    return v


def with_vertices(desc, v):
    d = desc.copy()
    d.vertices = np.ascontiguousarray(v, VERTEX_DTYPE).copy()
    return d


def tiny_scene(positions, triangles):
    """a few triangles in front of cube_scene's camera, under its light"""
    d = cube_scene(material_type=abi.MAT_UBER)
    v = np.zeros(len(positions), VERTEX_DTYPE)
    v["vv"] = np.asarray(positions, np.float32)
    v["vn"] = (0.0, 0.0, -1.0)
    v["vt"] = v["vv"][:, :2] * 0.5 + 0.5
    idx = np.asarray(triangles, np.uint32).reshape(-1)
    d.vertices, d.indices = v, idx
    d.meshes = np.array([(0, 2, 0, idx.size)], MESH_DTYPE)
    d.lights.append(make_light(abi.LIGHT_SUN, "sun", direction=(0.1, -0.3, 0.9), intensity=0.8))
    return d


def check_update(instance, desc, v1, levels="flat", builder="auto", mode="refit", first=0, size=(64, 48), renders=({},), rays=200_000):
    """A (created with desc, updated to v1[first:]) against B (created with v1): records, bounds and grid, hits, renders"""
    a = make_scene(instance, desc, levels, builder)
    ra = glaze_amd.RayTraceRenderer.new(instance, a, *size)
    ra.update_vertices(v1[first:], first=first, mode=mode)
    b = make_scene(instance, with_vertices(desc, v1), levels, builder)
    rb = glaze_amd.RayTraceRenderer.new(instance, b, *size)
    assert np.array_equal(tris_by_world_id(a), tris_by_world_id(b))
    assert_same_bounds_and_grid(a, b)
    assert_same_hits(a, b, rays)
    for kw in renders:
        assert_same_render(ra, rb, **kw)
    return a, b, ra, rb


# ---- 1: identity ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("levels,builder", [("flat", "lbvh"), ("flat", "ploc"), ("flat", "sah"), ("two_level", "auto")])
def test_identity_refit_reproduces_the_builders_bytes(instance, levels, builder):
    desc = instanced_sheets(12, seed=1) if levels == "two_level" else with_vertices(sheet_scene(), waved(sheet_scene().vertices))
    a = make_scene(instance, desc, levels, builder)
    before = structure(a)
    r = glaze_amd.RayTraceRenderer.new(instance, a, 64, 48)
    r.update_vertices(desc.vertices)
    assert_same_bytes(before, structure(a))
    u = r.geometry_update_info()
    assert u.box_area_built > 0 and u.box_area == pytest.approx(u.box_area_built, rel=1e-5)


# ---- 2: round trip -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("levels", ["flat", "two_level"])
def test_round_trip_returns_to_the_builds_bytes_without_drift(instance, levels):
    desc = instanced_sheets(12, seed=2) if levels == "two_level" else sheet_scene()
    first = 0 if levels == "two_level" else N_ROOM
    v0, v1 = desc.vertices, waved(desc.vertices, 0.2, 0.3)
    a = make_scene(instance, desc, levels)
    built = structure(a)
    r = glaze_amd.RayTraceRenderer.new(instance, a, 64, 48)
    r.update_vertices(v1[first:], first=first)
    moved = structure(a)
    assert not np.array_equal(moved["tris"], built["tris"]) and not np.array_equal(moved["nodes"], built["nodes"])
    r.update_vertices(v0[first:], first=first)
    assert_same_bytes(built, structure(a))
    for _ in range(5):                                                                          # ten alternations
        r.update_vertices(v1[first:], first=first)
        r.update_vertices(v0[first:], first=first)
    r.update_vertices(v1[first:], first=first)
    assert_same_bytes(moved, structure(a))


# ---- 3: moved, flattened -------------------------------------------------------------------------------------------------------
def assert_boxes_contain_their_triangles(scene):
    """every child box of the 4-wide nodes, de-quantised, contains the padded boxes of all triangles below it"""
    nodes, tris = scene.debug_bvh()
    i = scene.info()
    glo, cell = np.array(i.bvh_grid_lo, np.float64), np.array(i.bvh_grid_cell, np.float64)
    flags = tris.view(np.uint32)[:, 11]
    corners = tris[:, [0, 1, 2, 4, 5, 6, 8, 9, 10]].reshape(-1, 3, 3)
    tlo, thi = corners.min(1), corners.max(1)
    pad = np.float32(1e-5) * np.maximum(np.maximum(np.abs(tlo), np.abs(thi)), np.float32(1e-3))
    tlo, thi = (tlo - pad).astype(np.float64), (thi + pad).astype(np.float64)
    n = nodes.shape[0]
    sub_lo, sub_hi = np.full((n, 3), np.inf), np.full((n, 3), -np.inf)
    for node in range(n - 1, -1, -1):                                                           # children have higher numbers
        for k in range(4):
            link = int(nodes[node, 12 + k].astype(np.int32))
            if link == 0x7FFFFFFF:
                continue
            if link < 0:
                slot = ~link
                last = slot + (1 if flags[slot] & HAS_PARTNER else 0)
                lo, hi = tlo[slot:last + 1].min(0), thi[slot:last + 1].max(0)
            else:
                assert link > node
                lo, hi = sub_lo[link], sub_hi[link]
            w = nodes[node, 3 * k:3 * k + 3].astype(np.int64)
            qlo, qhi = glo + (w & 0xFFFF) * cell, glo + (w >> 16) * cell
            assert (qlo <= lo).all() and (qhi >= hi).all(), (node, k)
            sub_lo[node], sub_hi[node] = np.minimum(sub_lo[node], lo), np.maximum(sub_hi[node], hi)


@pytest.mark.parametrize("builder", ["lbvh", "ploc", "sah"])
def test_moved_sheet_equals_a_fresh_scene(instance, builder):
    desc = sheet_scene()
    v1 = waved(desc.vertices, 0.2, 0.5)
    renders = [dict(mode=m, chains=c, width=w) for m, c, w in (("auto", 0, 0), ("two_kernels", 1, 4), ("two_kernels", 3, 8), ("path", 1, 4), ("path", 3, 8))]
    a, b, ra, _ = check_update(instance, desc, v1, "flat", builder, first=N_ROOM, renders=renders)
    assert a.debug_bvh8().shape[0] > 0 and a.debug_leaf_records().shape[0] > 256
    assert_boxes_contain_their_triangles(a)
    u = ra.geometry_update_info()
    assert (u.mode, u.meshes_touched) == (abi.GEOMETRY_REFIT, 1) and u.update_ms >= 0 and u.box_area > 0 and u.box_area_built > 0


# ---- 4: the small shapes -------------------------------------------------------------------------------------------------------
QUAD = [(-0.5, -0.5, 2.0), (0.5, -0.5, 2.0), (0.5, 0.5, 2.0), (-0.5, 0.5, 2.0)]


def moved_positions(desc, fn):
    v = desc.vertices.copy()
    v["vv"] = fn(v["vv"].astype(np.float64)).astype(np.float32)
    return v


def test_one_triangle(instance):
    desc = tiny_scene(QUAD[:3], [0, 1, 2])
    v1 = moved_positions(desc, lambda p: p * (1.5, 0.7, 1.0) + (0.2, 0.1, 0.5))
    a, *_ = check_update(instance, desc, v1)
    assert a.debug_bvh()[0].shape[0] == 1 and a.debug_leaf_records().shape[0] == 1


@pytest.mark.parametrize("second,swapped", [((0, 2, 3), False), ((0, 3, 1), True)])
def test_one_quad_leaf_in_both_vertex_orders(instance, second, swapped):
    desc = tiny_scene(QUAD if not swapped else [QUAD[0], QUAD[2], QUAD[3], QUAD[1]], [0, 1, 2, *second])
    a = make_scene(instance, desc)
    leaves = a.debug_leaf_records()
    assert leaves.shape[0] == 1 and bool(leaves[0, 11] & HAS_PARTNER) and bool(leaves[0, 11] & QUAD_SWAPPED) == swapped
    v1 = moved_positions(desc, lambda p: p + np.stack([0.1 * p[:, 1], 0.2 * p[:, 0], 0.3 * p[:, 0] * p[:, 1]], -1))
    check_update(instance, desc, v1)


def test_folded_quads_stay_paired_in_the_refit_and_not_in_a_fresh_build(instance):
    desc = sheet_scene(room=False)
    v1 = desc.vertices.copy()
    n = 33
    rows, cols = np.divmod(np.arange(n * n), n)
    # One corner off the shared diagonal pulled far up in a quarter of the cells: that triangle's box becomes tall, its partner's stays
    # flat, and the joint box costs more than the builder's area rule allows.  (Lifting both off-diagonal corners would not do: each
    # triangle's box then spans the whole cell, and the rule, which sees boxes, still pairs them.)
    v1["vv"][:, 1] += np.where((rows % 2 == 1) & (cols % 2 == 0), 0.5, 0.0).astype(np.float32)
    a, b, *_ = check_update(instance, desc, v1)
    assert a.debug_leaf_records().shape[0] == 1024 and b.debug_leaf_records().shape[0] > 1024   # A keeps its pairs, the builder would not form them


@pytest.mark.parametrize("factor", [3.0, 0.1])
def test_bounds_grow_and_shrink_and_the_grid_follows(instance, factor):
    desc = sheet_scene()
    v1 = moved_positions(with_vertices(desc, waved(desc.vertices)), lambda p: p * factor)
    a, b, *_ = check_update(instance, desc, v1)
    assert np.array(a.info().bvh_grid_cell) == pytest.approx(np.array(make_scene(instance, desc).info().bvh_grid_cell) * factor, rel=0.2)


@pytest.mark.parametrize("flatten", [True, False])
def test_a_thick_sheet_made_flat_and_a_flat_one_made_thick(instance, flatten):
    flat = sheet_scene(room=False)
    flat.vertices["vv"][:, 1] = 0.0
    thick = with_vertices(flat, waved(flat.vertices, 0.2, 0.1, first=0))
    desc, v1 = (thick, flat.vertices) if flatten else (flat, thick.vertices)
    a, b, *_ = check_update(instance, desc, v1)
    if flatten:
        assert a.info().bounds_max[1] - a.info().bounds_min[1] < 1e-6                             # nothing but the pad left across y


# ---- 5: attributes only --------------------------------------------------------------------------------------------------------
def test_new_normals_and_texture_coordinates_leave_the_structure_alone(instance):
    desc = sheet_scene(opacity=True)
    v1 = desc.vertices.copy()
    v1["vn"][N_ROOM:] = waved(desc.vertices, 0.3)["vn"][N_ROOM:]
    v1["vt"][N_ROOM:] = v1["vt"][N_ROOM:, ::-1] * 2.0 + 0.25
    a = make_scene(instance, desc)
    before = structure(a)
    a2, b, *_ = check_update(instance, desc, v1, first=N_ROOM, renders=[dict(mode="two_kernels"), dict(mode="path")])
    assert_same_bytes(before, structure(a2))
    ra = glaze_amd.RayTraceRenderer.new(instance, a, 64, 48)
    unchanged = render(ra)[0]
    ra.update_vertices(v1)
    assert not np.array_equal(bits(unchanged), bits(render(ra)[0]))                               # the alpha test and the shading did see them


def test_an_emissive_sheet_lights_the_room_from_where_it_is_now(instance):
    desc = sheet_scene(emissive=True)
    check_update(instance, desc, waved(desc.vertices, 0.25, 1.0), first=N_ROOM, rays=20_000, renders=[dict(depth=5), dict(depth=5, mode="path")])


# ---- 6: two levels -------------------------------------------------------------------------------------------------------------
def instanced_sheets(n, seed=0):
    """two meshes (the cube and the sheet) under the room and n randomly placed instances"""
    rng = np.random.default_rng(seed)
    d = sheet_scene()
    d.transforms = np.concatenate([col_major(np.eye(4))[None], random_transforms(rng, n)])
    d.instances = np.array([(0, 0)] + [(i % 2, 1 + i) for i in range(n)], INSTANCE_DTYPE)
    return d


def tlas_field(scene, byte):
    return scene.debug_tlas_instances().reshape(-1, 192)[:, byte:byte + 4].copy().view(np.uint32).ravel()


def cube_mesh_records(scene):
    """the cube mesh's nodes and leaf records (mesh 0: the first in both arrays; the sheet's follow)"""
    node_base, quad_base = tlas_field(scene, 88), tlas_field(scene, 176)
    sheet_nodes, sheet_quads = node_base[quad_base != 0].min(), quad_base[quad_base != 0].min()
    return scene.debug_bvh()[0][node_base.min():sheet_nodes], scene.debug_leaf_records()[:sheet_quads]


def test_two_level_full_update_equals_a_fresh_scene(instance):
    desc = instanced_sheets(40, seed=3)
    a, b, ra, _ = check_update(instance, desc, waved(desc.vertices, 0.2, 0.4, first=0), "two_level")
    assert a.info().as_levels == b.info().as_levels == 2 and ra.geometry_update_info().meshes_touched == 2


def test_two_level_partial_update_refits_the_sheet_alone(instance):
    desc = instanced_sheets(40, seed=4)
    v1 = waved(desc.vertices, 0.2, 0.7)
    before = cube_mesh_records(make_scene(instance, desc, "two_level"))
    a, b, ra, _ = check_update(instance, desc, v1, "two_level", first=N_ROOM)
    assert ra.geometry_update_info().meshes_touched == 1
    for x, y in zip(before, cube_mesh_records(a)):
        assert x.size and np.array_equal(x, y)
    for x, y in zip(a.debug_instance_boxes(True), a.debug_instance_boxes(False)):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))


@pytest.mark.parametrize("vertices_first", [True, False])
def test_vertex_and_transform_updates_in_either_order(instance, vertices_first):
    desc = instanced_sheets(40, seed=5)
    v1 = waved(desc.vertices, 0.2, 0.9)
    t1 = desc.transforms.copy()
    t1[1:] = random_transforms(np.random.default_rng(6), 40)
    a = make_scene(instance, desc, "two_level")
    ra = glaze_amd.RayTraceRenderer.new(instance, a, 64, 48)
    for step in (0, 1) if vertices_first else (1, 0):
        ra.update_transforms(t1) if step else ra.update_vertices(v1[N_ROOM:], first=N_ROOM)
    both = with_vertices(desc, v1)
    both.transforms = t1
    b = make_scene(instance, both, "two_level")
    assert_same_hits(a, b)
    assert_same_render(ra, glaze_amd.RayTraceRenderer.new(instance, b, 64, 48))


# ---- 7: rebuild mode -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("levels", ["flat", "two_level"])
def test_rebuild_mode_is_a_fresh_build(instance, levels):
    desc = instanced_sheets(20, seed=7)
    a, b, ra, _ = check_update(instance, desc, waved(desc.vertices, 0.2, 1.1), levels, mode="rebuild", first=N_ROOM, rays=50_000)
    assert_same_structure(a, b)
    u = ra.geometry_update_info()
    assert u.mode == abi.GEOMETRY_REBUILD and u.box_area == pytest.approx(u.box_area_built, rel=1e-5) and u.box_area > 0


# ---- 8: interface --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("levels", ["flat", "two_level"])
def test_refused_arguments_change_nothing(instance, levels):
    desc = instanced_sheets(10, seed=8)
    a = make_scene(instance, desc, levels)
    r = glaze_amd.RayTraceRenderer.new(instance, a, 64, 48)
    ref = glaze_amd.RayTraceRenderer.new(instance, make_scene(instance, desc, levels), 64, 48)
    for x in (r, ref):
        x.set_depth(4)
        x.set_seed(5)
        x.step(3)
    before = structure(a)
    with pytest.raises(glaze_amd.GlazeError) as e:
        r.geometry_update_info()                                                                 # no update yet
    assert e.value.status == abi.E_ARG
    v = np.ascontiguousarray(waved(desc.vertices)).view(np.float32).reshape(-1, 8)
    n = v.shape[0]
    call = abi.lib().glz_renderer_update_vertices
    assert call(r._h, None, 0, n, abi.GEOMETRY_REFIT) == abi.E_ARG                              # null
    assert call(r._h, v.ctypes.data, 0, 0, abi.GEOMETRY_REFIT) == abi.E_ARG                     # none
    assert call(r._h, v.ctypes.data, 1, n, abi.GEOMETRY_REFIT) == abi.E_ARG                     # past the end
    assert call(r._h, v.ctypes.data, 0xFFFFFFFF, 2, abi.GEOMETRY_REFIT) == abi.E_ARG            # (a sum that wraps in 32 bits)
    assert call(r._h, v.ctypes.data, 0, n, 2) == abi.E_ARG                                      # unknown mode
    with pytest.raises(ValueError):
        r.update_vertices(v[:, :3])
    assert_same_bytes(before, structure(a))
    for x in (r, ref):
        x.step(4)
    assert np.array_equal(bits(r.read_hdr()), bits(ref.read_hdr()))
    assert np.array_equal(bits(r.read_result()), bits(ref.read_result()))


# (The update acts on the scene object, so whoever holds the scene sees it: every case above traces A through the SCENE handle after
# updating through the renderer.  Two renderers on one scene cannot be had through the C interface -- glz_renderer_create takes the
# scene over and refuses one that belongs to a renderer -- so there is no such case here.)


def test_an_abi_vertex_array_is_taken_as_it_is(instance):
    desc = tiny_scene(QUAD, [0, 1, 2, 0, 2, 3])
    v1 = moved_positions(desc, lambda p: p * (0.5, 1.2, 1.0))
    arr = (abi.Vertex * len(v1)).from_buffer_copy(np.ascontiguousarray(v1).tobytes())
    a = make_scene(instance, desc)
    glaze_amd.RayTraceRenderer.new(instance, a, 64, 48).update_vertices(arr)
    assert np.array_equal(tris_by_world_id(a), tris_by_world_id(make_scene(instance, with_vertices(desc, v1))))


@pytest.fixture
def loopback(monkeypatch):
    monkeypatch.setenv("GLAZE_MULTI_LOOPBACK", "1")


@pytest.mark.parametrize("levels", ["flat", "two_level"])
def test_loopback_devices_follow_a_vertex_update(instance, loopback, levels):
    desc = instanced_sheets(10, seed=9)
    v1 = waved(desc.vertices, 0.2, 1.5)
    r = glaze_amd.RayTraceRenderer.new(instance, make_scene(instance, desc, levels), 136, 200)
    r.set_devices([instance.device] * 2)
    r.update_vertices(v1[N_ROOM:], first=N_ROOM)
    one = glaze_amd.RayTraceRenderer.new(instance, make_scene(instance, with_vertices(desc, v1), levels), 136, 200)
    assert_same_render(r, one)
    assert np.array_equal(r.read_rgba8(), one.read_rgba8())


# ---- 9: one oracle render ------------------------------------------------------------------------------------------------------
def test_refitted_render_matches_the_oracle(instance):
    desc = sheet_scene()
    v1 = waved(desc.vertices, 0.2, 1.7)
    r = glaze_amd.RayTraceRenderer.new(instance, make_scene(instance, desc), 32, 24)
    r.update_vertices(v1[N_ROOM:], first=N_ROOM)
    img, _ = render(r, 5, seed=7, depth=4)
    o = OracleRenderer(OracleScene(with_vertices(desc, v1)), 32, 24)
    o.set_depth(4)
    o.set_seed(7)
    o.step(5)
    assert np.array_equal(bits(img), bits(o.read_hdr()))
