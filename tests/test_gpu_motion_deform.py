"""Motion vectors and reprojection that follow deforming meshes (glz_renderer_read_motion_from, glz_renderer_reproject_from; the rule
"with previous vertices" of the motion plane's specification in include/glaze_abi.h).

V0 is the previous vertex set, V1 the current one.  The plane must equal test_gpu_motion.py's float64 restatement on the oracle's hits of
the CURRENT scene with the PREVIOUS positions put in, within that file's bounds (the arithmetic has the operation count of the rigid
case); it must not depend on how the scene came to hold V1 (created with it, refitted, rebuilt, by which builder, in one level or two); it
must be plain read_motion's, bit for bit, wherever the previous positions are the current ones; and a binary32 restatement of the rule in
numpy must reproduce it bit for bit."""
import ctypes as C

import numpy as np
import pytest

import glaze_amd
from glaze_amd import abi
from glaze_amd.scene_desc import make_camera
from glaze_amd.scenes import atrium_scene

from denoise_ref import synthetic_frame
from reproject_ref import bits, projection_bounds
from test_gpu_motion import check_motion, focal, moved_camera, moved_transforms, oracle_hits, restate_motion, wall_and_card, world_points, D1, FOVX
from test_gpu_vertex_update import N_ROOM, QUAD, instanced_sheets, sheet_scene, tiny_scene, waved, with_vertices

pytestmark = pytest.mark.gpu

W, H = 128, 72
MISS = 0xFFFFFFFF
HAS_PARTNER, QUAD_SWAPPED = 0x40000000, 0x20000000
SHEET = 1                                             # the sheet's instance in sheet_scene()


def make_scene(instance, desc, levels="flat", builder="auto"):
    instance.set_as_levels(levels)
    instance.set_bvh_builder(builder)
    try:
        return glaze_amd.RayTraceScene.from_desc(instance, desc)
    finally:
        instance.set_as_levels("auto")
        instance.set_bvh_builder("auto")


def renderer(instance, desc, levels="flat", builder="auto", size=(W, H)):
    return glaze_amd.RayTraceRenderer.new(instance, make_scene(instance, desc, levels, builder), *size)


def updated(instance, desc, v1, first, mode, levels="flat", builder="auto", size=(W, H)):
    """a renderer on a scene created with desc's vertices and updated to v1[first:]"""
    r = renderer(instance, desc, levels, builder, size)
    r.update_vertices(v1[first:], first=first, mode=mode)
    return r


def sheet_desc():
    """sheet_scene() under a camera that looks down at the sheet"""
    d = sheet_scene()
    d.camera = make_camera(position=(0, 0.35, -0.35), target=(0, -0.4, 0.55), fovx=FOVX, near=1e-3, far=100.0)
    return d


def hit_triangles(desc, hits):
    """per ray: the hit mask, the hit triangle's three entries of the index buffer in index-buffer order (0 for a miss), its transform id"""
    t, tri, inst, _, _ = hits
    hit = np.isfinite(t)
    meshes = {int(m["id"]): m for m in desc.meshes}
    inst_mesh = [meshes[int(i["mesh_id"])] for i in desc.instances]
    counts = np.array([int(m["index_count"]) // 3 for m in inst_mesh], np.int64)
    base = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    ii = np.where(hit, inst, 0).astype(np.int64)
    local = np.where(hit, tri.astype(np.int64) - base[ii], 0)
    first = np.array([int(m["index_offset"]) for m in inst_mesh], np.int64)[ii] + 3 * local
    vid = np.stack([desc.indices[first + k] for k in range(3)], -1).astype(np.int64)
    xf = np.array([int(i["transform_id"]) for i in desc.instances], np.int64)[ii]
    return hit, vid, xf


def pixels_apart(a, b):
    """the distance in pixels between two restated planes where both are valid (0 elsewhere)"""
    both = a[2] & b[2]
    d = np.hypot(a[0][:, 0] - b[0][:, 0], a[0][:, 1] - b[0][:, 1])
    return np.where(both, d, 0.0)


def outside_bound(got, restated):
    """per pixel: a valid pixel of the restatement at which `got` misses check_motion's bound on fx or fy"""
    plane, _, valid, _, (bx, by, _) = restated
    g = got.reshape(-1, 4).astype(np.float64)
    with np.errstate(invalid="ignore"):
        return valid & ((np.abs(g[:, 0] - plane[:, 0]) > bx) | (np.abs(g[:, 1] - plane[:, 1]) > by))


# ---------------------------------------------------------------------------------------------------------------------
# 1. the restatement on a flattened scene, however the scene came to hold V1
# ---------------------------------------------------------------------------------------------------------------------
def test_deformed_sheet_equals_the_restatement_however_the_scene_was_made(instance):
    desc0 = sheet_desc()
    v0, v1 = desc0.vertices, waved(desc0.vertices, 0.2, 0.5)
    desc1 = with_vertices(desc0, v1)
    prev_cam = moved_camera(desc1.camera)
    fresh = renderer(instance, desc1)
    hits = oracle_hits(desc1, fresh)
    restated = restate_motion(with_vertices(desc1, v0), hits, prev_cam, desc1.transforms, W, H)
    rigid = restate_motion(desc1, hits, prev_cam, desc1.transforms, W, H)
    on_sheet = restated[3] == SHEET
    moving = on_sheet & (pixels_apart(restated, rigid) > 1.0)
    plain = fresh.read_motion(prev_cam)
    wrong = outside_bound(plain, restated) & moving
    print("sheet: %d pixels, %d with restated motion more than 1 px from the rigid one (median %.2f px); plain read_motion misses the bound on %d of them" % (
        on_sheet.sum(), moving.sum(), np.median(pixels_apart(restated, rigid)[moving]), wrong.sum()))
    assert moving.sum() >= 3000
    assert wrong.sum() >= moving.sum() / 2                                             # without the previous vertices the plane is wrong there
    prev = dict(prev_vertices=v0[N_ROOM:], first_vertex=N_ROOM)
    planes = {"created with V1": fresh.read_motion(prev_cam, **prev),
              "refit": updated(instance, desc0, v1, N_ROOM, "refit").read_motion(prev_cam, **prev),
              "rebuild": updated(instance, desc0, v1, N_ROOM, "rebuild").read_motion(prev_cam, **prev)}
    for builder in ("lbvh", "ploc", "sah"):
        planes["refit, " + builder] = updated(instance, desc0, v1, N_ROOM, "refit", builder=builder).read_motion(prev_cam, **prev)
    for name, plane in planes.items():
        check_motion("sheet, " + name, plane, restated)
        assert np.array_equal(bits(plane), bits(planes["created with V1"])), name    # hits do not depend on the tree


# ---------------------------------------------------------------------------------------------------------------------
# 2. part of a mesh: the range ends inside triangles
# ---------------------------------------------------------------------------------------------------------------------
def test_a_range_that_covers_part_of_a_mesh(instance):
    desc0 = sheet_desc()
    first = N_ROOM + 544                                                               # the second half of the sheet's 1 089 vertices
    v1 = waved(desc0.vertices, 0.2, 0.5)
    mixed = v1.copy()
    mixed[first:] = desc0.vertices[first:]                                             # the previous state: V0 there, V1 elsewhere
    desc1 = with_vertices(desc0, v1)
    prev_cam = moved_camera(desc1.camera)
    ren = renderer(instance, desc1)
    hits = oracle_hits(desc1, ren)
    restated = restate_motion(with_vertices(desc1, mixed), hits, prev_cam, desc1.transforms, W, H)
    rigid = restate_motion(desc1, hits, prev_cam, desc1.transforms, W, H)
    hit, vid, _ = hit_triangles(desc1, hits)
    touched = hit & (vid >= first).any(-1)
    both_sides = touched & (vid < first).any(-1)
    moving = touched & (pixels_apart(restated, rigid) > 1.0)
    print("half the sheet: %d pixels on touched triangles, %d of them moving by more than 1 px, %d on triangles with indices on both sides of the range's start" % (
        touched.sum(), moving.sum(), both_sides.sum()))
    assert moving.sum() >= 1500 and both_sides.sum() >= 50
    check_motion("half the sheet", ren.read_motion(prev_cam, prev_vertices=desc0.vertices[first:], first_vertex=first), restated)


# ---------------------------------------------------------------------------------------------------------------------
# 3. two levels: instances moved and meshes deformed at once
# ---------------------------------------------------------------------------------------------------------------------
def two_level_case():
    desc0 = instanced_sheets(12, seed=1)
    v1 = waved(desc0.vertices, 0.2, 0.4, first=0)                                      # both meshes deform
    return desc0, v1, with_vertices(desc0, v1), moved_transforms(desc0.transforms, seed=4, every=3), moved_camera(desc0.camera)


def test_two_levels_moved_and_deformed_at_once(instance):
    desc0, v1, desc1, prev_xf, prev_cam = two_level_case()
    fresh = renderer(instance, desc1, "two_level")
    assert fresh.scene.info().as_levels == 2
    hits = oracle_hits(desc1, fresh)
    restated = restate_motion(desc0, hits, prev_cam, prev_xf, W, H)                    # desc0 is desc1 with V0 in it
    rigid = restate_motion(desc1, hits, prev_cam, prev_xf, W, H)
    moving = pixels_apart(restated, rigid) > 1.0
    print("instanced sheets: %d hit pixels, %d moving by more than 1 px" % (restated[1].sum(), moving.sum()))
    assert restated[1].all() and moving.sum() >= 6000
    prev = dict(prev_transforms=prev_xf, prev_vertices=desc0.vertices, first_vertex=0)
    plane = fresh.read_motion(prev_cam, **prev)
    check_motion("instanced sheets, two levels", plane, restated)
    refit = updated(instance, desc0, v1, 0, "refit", "two_level")
    assert refit.scene.info().as_levels == 2
    assert np.array_equal(bits(refit.read_motion(prev_cam, **prev)), bits(plane))
    flat = renderer(instance, desc1, "flat")
    assert flat.scene.info().as_levels == 1
    assert np.array_equal(bits(flat.read_motion(prev_cam, **prev)), bits(plane))


# ---------------------------------------------------------------------------------------------------------------------
# 4. the smallest shapes
# ---------------------------------------------------------------------------------------------------------------------
def moved_positions(desc, fn):
    v = desc.vertices.copy()
    v["vv"] = fn(v["vv"].astype(np.float64)).astype(np.float32)
    return v


def small_cases():
    sheared = lambda p: p + np.stack([0.1 * p[:, 1], 0.2 * p[:, 0], 0.3 * p[:, 0] * p[:, 1]], -1)   # noqa: E731
    return {"one triangle": (lambda: tiny_scene(QUAD[:3], [0, 1, 2]), lambda p: p * (1.5, 0.7, 1.0) + (0.2, 0.1, 0.5), None),
            "one quad leaf": (lambda: tiny_scene(QUAD, [0, 1, 2, 0, 2, 3]), sheared, False),
            "one quad leaf, swapped": (lambda: tiny_scene([QUAD[0], QUAD[2], QUAD[3], QUAD[1]], [0, 1, 2, 0, 3, 1]), sheared, True)}


@pytest.mark.parametrize("name", list(small_cases()))
def test_the_smallest_scenes(instance, name):
    make, fn, swapped = small_cases()[name]
    desc = make()
    ren = renderer(instance, desc)
    leaves = ren.scene.debug_leaf_records()
    assert leaves.shape[0] == 1
    if swapped is None:
        assert ren.scene.debug_bvh()[0].shape[0] == 1                                  # one triangle, one node
    else:
        assert bool(leaves[0, 11] & HAS_PARTNER) and bool(leaves[0, 11] & QUAD_SWAPPED) == swapped
    before = moved_positions(desc, fn)
    prev_cam = moved_camera(desc.camera, shift=(0.05, 0.02, -0.04), turn=(0.05, -0.02, 0.0))
    hits = oracle_hits(desc, ren)
    assert np.isfinite(hits[0]).sum() > 200
    check_motion(name, ren.read_motion(prev_cam, prev_vertices=before), restate_motion(with_vertices(desc, before), hits, prev_cam, desc.transforms, W, H))


def test_a_frame_whose_last_block_is_part_empty(instance):
    w, h = 97, 61                                                                      # 5 917 pixels: 23 blocks of 256 and 29 threads of the next
    desc0 = sheet_desc()
    v1 = waved(desc0.vertices, 0.2, 0.5)
    desc1 = with_vertices(desc0, v1)
    prev_cam = moved_camera(desc1.camera)
    ren = renderer(instance, desc1, size=(w, h))
    hits = oracle_hits(desc1, ren)
    got = ren.read_motion(prev_cam, prev_vertices=desc0.vertices[N_ROOM:], first_vertex=N_ROOM)
    assert got.shape == (h, w, 4)
    check_motion("97 x 61", got, restate_motion(desc0, hits, prev_cam, desc1.transforms, w, h))


# ---------------------------------------------------------------------------------------------------------------------
# 5. identities, bit for bit
# ---------------------------------------------------------------------------------------------------------------------
def read_motion_from(ren, prev_cam, transforms=None, vertices=None, first=0, count=None, expect=0):
    """glz_renderer_read_motion_from itself, whatever of the state is null; count: n_vertices if not the array's length"""
    t = None if transforms is None else np.ascontiguousarray(transforms, np.float32)
    v = None if vertices is None else np.ascontiguousarray(vertices).view(np.float32).reshape(-1, 8)
    state = abi.PreviousState(C.cast(C.byref(prev_cam), C.c_void_p), None if t is None else t.ctypes.data, 0 if t is None else t.shape[0],
                              None if v is None else v.ctypes.data, first, (0 if v is None else v.shape[0]) if count is None else count)
    out = np.full((ren.height, ren.width, 4), 7.0, np.float32)
    assert abi.lib().glz_renderer_read_motion_from(ren._h, C.byref(state), out.ctypes.data_as(C.c_void_p)) == expect
    return out


def test_previous_vertices_that_change_nothing_give_plain_read_motion(instance):
    desc0 = sheet_desc()
    v1 = waved(desc0.vertices, 0.2, 0.5)
    desc1 = with_vertices(desc0, v1)
    prev_cam = moved_camera(desc1.camera)
    ren = renderer(instance, desc1)
    plain = ren.read_motion(prev_cam)
    assert (bits(plain[..., 3]) == SHEET).sum() > 3000
    # the previous vertices are the current ones: the whole buffer, a range inside the sheet
    assert np.array_equal(bits(ren.read_motion(prev_cam, prev_vertices=v1)), bits(plain))
    assert np.array_equal(bits(ren.read_motion(prev_cam, prev_vertices=v1[N_ROOM + 100:N_ROOM + 700], first_vertex=N_ROOM + 100)), bits(plain))
    # no previous vertices through the new entry point, with and without transforms
    assert np.array_equal(bits(read_motion_from(ren, prev_cam)), bits(plain))
    assert np.array_equal(bits(read_motion_from(ren, prev_cam, desc1.transforms)), bits(plain))
    assert np.array_equal(bits(read_motion_from(ren, prev_cam, vertices=None, first=5)), bits(plain))   # (the range is ignored with them)
    # a range no visible triangle references: the sheet's, with the camera turned to the room's back wall
    away = make_camera(position=(0, 0, 0), target=(0, 0.2, -100), fovx=FOVX, near=1e-3, far=100.0)
    ren.update_camera(away)
    prev_away = moved_camera(away, shift=(0.1, 0.05, 0.1), turn=(0.3, 0.0, 0.0))
    plain = ren.read_motion(prev_away)
    ids = bits(plain[..., 3])
    assert (ids == 0).all()                                                            # the room alone
    assert np.array_equal(bits(ren.read_motion(prev_away, prev_vertices=desc0.vertices[N_ROOM:], first_vertex=N_ROOM)), bits(plain))


# ---------------------------------------------------------------------------------------------------------------------
# 6. the rule restated in binary32
# ---------------------------------------------------------------------------------------------------------------------
def restate_binary32(desc, positions, hits, prev_cam, prev_transforms, w, h):
    """The motion plane's specification in numpy float32, every operation rounded on its own and in the header's order: b0 = (1 - u) - v,
    P_obj = (v0*b0 + v1*u) + v2*v from `positions` (all the scene's vertices, float32), P' = the previous matrix's rows summed left to
    right, host_project_points under the previous camera.  Returns the plane's words (n x 4 uint32)."""
    f = np.float32
    _, _, inst, u, v = hits
    hit, vid, xf = hit_triangles(desc, hits)
    u, v = np.where(hit, u, 0).astype(f), np.where(hit, v, 0).astype(f)
    b0 = (f(1.0) - u) - v
    vv = np.asarray(positions, f)[vid]                                                 # n x 3 x 3
    p = (vv[:, 0] * b0[:, None] + vv[:, 1] * u[:, None]) + vv[:, 2] * v[:, None]
    m = np.asarray(prev_transforms, f).reshape(-1, 16)[xf]
    world = np.stack([((m[:, r] * p[:, 0] + m[:, 4 + r] * p[:, 1]) + m[:, 8 + r] * p[:, 2]) + m[:, 12 + r] for r in range(3)], -1)
    assert p.dtype == world.dtype == f
    proj = glaze_amd.host_project_points(prev_cam, w, h, world)
    py, px = np.divmod(np.arange(w * h), w)
    valid = hit & np.isfinite(proj[:, 2])
    plane = np.zeros((w * h, 4), f)
    plane[:, 0] = np.where(valid, proj[:, 0] - (px.astype(f) + f(0.5)), f(0))
    plane[:, 1] = np.where(valid, proj[:, 1] - (py.astype(f) + f(0.5)), f(0))
    plane[:, 2] = np.where(valid, proj[:, 2], f(np.inf))
    words = bits(plane).copy()
    words[:, 3] = np.where(hit, inst, np.uint32(MISS)).astype(np.uint32)
    return words


def differing(got, words):
    return int((bits(got).reshape(-1, 4) != words).any(-1).sum())


def test_the_rule_in_binary32_gives_the_planes_bits(instance):
    # flattened: the sheet of test 1
    desc0 = sheet_desc()
    desc1 = with_vertices(desc0, waved(desc0.vertices, 0.2, 0.5))
    prev_cam = moved_camera(desc1.camera)
    prev_xf = moved_transforms(desc1.transforms, seed=4)
    ren = renderer(instance, desc1)
    hits = oracle_hits(desc1, ren)
    control = differing(ren.read_motion(prev_cam, prev_xf), restate_binary32(desc1, desc1.vertices["vv"], hits, prev_cam, prev_xf, W, H))
    deform = differing(ren.read_motion(prev_cam, prev_xf, prev_vertices=desc0.vertices[N_ROOM:], first_vertex=N_ROOM),
                       restate_binary32(desc1, desc0.vertices["vv"], hits, prev_cam, prev_xf, W, H))
    print("sheet: pixels that differ from the binary32 restatement: rigid (control) %d, deforming %d" % (control, deform))
    assert control == 0                                                                # plain read_motion: holds without previous vertices too
    assert deform == 0
    # two levels: the instanced sheets of test 3
    desc0, v1, desc1, prev_xf, prev_cam = two_level_case()
    ren = renderer(instance, desc1, "two_level")
    hits = oracle_hits(desc1, ren)
    control = differing(ren.read_motion(prev_cam, prev_xf), restate_binary32(desc1, desc1.vertices["vv"], hits, prev_cam, prev_xf, W, H))
    deform = differing(ren.read_motion(prev_cam, prev_xf, prev_vertices=desc0.vertices), restate_binary32(desc1, desc0.vertices["vv"], hits, prev_cam, prev_xf, W, H))
    print("instanced sheets: pixels that differ from the binary32 restatement: rigid (control) %d, deforming %d" % (control, deform))
    assert control == 0
    assert deform == 0


# ---------------------------------------------------------------------------------------------------------------------
# 7. closed form: the card's vertices shifted sideways
# ---------------------------------------------------------------------------------------------------------------------
def test_closed_form_shifted_card(instance):
    """The camera sits at the origin and looks down -z with y up, so a point's pixel is F (X, -Y) / depth from the image centre (y down on
    screen).  The card's PREVIOUS vertices at current + (3.5 D1 / F, -2.5 D1 / F, 0) therefore give its pixels a motion of (+3.5, +2.5) px.
    (The shift has the magnitudes the issue names, dx = 3.5 D1 / F and dy = 2.5 D1 / F, with the signs that give the expected (3.5, 2.5):
    the signs of test_closed_form_camera_translation are those of a moved EYE, which moves the image the other way.)  z' is the distance
    of the shifted point from the eye; the wall's pixels keep the plane of the static case, bit for bit."""
    desc = wall_and_card()
    ren = renderer(instance, desc, "auto")
    fpx, c2s = focal(desc.camera)
    sx, sy = 3.5 * D1 / fpx, -2.5 * D1 / fpx
    n_card = 4
    before = desc.vertices[-n_card:].copy()
    assert np.allclose(before["vv"][:, 2], -D1)                                        # the card's vertices are the last four
    before["vv"] = (before["vv"].astype(np.float64) + (sx, sy, 0.0)).astype(np.float32)
    first = len(desc.vertices) - n_card
    static = ren.read_motion(desc.camera)
    m = ren.read_motion(desc.camera, prev_vertices=before, first_vertex=first)
    ids = bits(m[..., 3])
    wall, card = ids == 0, ids == 1
    assert wall.sum() + card.sum() == W * H and card.sum() > 300
    assert np.array_equal(bits(m[wall]), bits(static[wall]))
    P = world_points(m[..., 3], fpx)
    P_prev = P + np.where(card[..., None], (float(np.float32(sx)), float(np.float32(sy)), 0.0), 0.0)
    bx, by, bz = projection_bounds(c2s, True, W, H, P_prev.reshape(-1, 3), (0, 0, 0), -P_prev.reshape(-1, 3)[:, 2], None)
    bx, by, bz = bx.reshape(H, W), by.reshape(H, W), bz.reshape(H, W)
    ex, ey = np.abs(m[..., 0] - np.where(card, 3.5, 0.0)), np.abs(m[..., 1] - np.where(card, 2.5, 0.0))
    z_want = np.linalg.norm(P_prev, axis=-1)
    ez = np.abs(m[..., 2] - z_want) / z_want
    print("shifted card: largest error / bound: x %.3f, y %.3f, z' %.3f" % ((ex / bx).max(), (ey / by).max(), (ez / bz).max()))
    assert (ex <= bx).all() and (ey <= by).all() and (ez <= bz).all()
    # the same shift as the card's previous TRANSFORM
    shift = np.eye(4)
    shift[:3, 3] = (sx, sy, 0.0)
    prev_xf = np.stack([np.eye(4).T.reshape(16), shift.T.reshape(16)]).astype(np.float32)
    t = ren.read_motion(desc.camera, prev_xf)
    assert np.array_equal(bits(t[..., 3]), ids)
    assert (np.abs(t[..., 0] - m[..., 0]) <= 2 * bx).all() and (np.abs(t[..., 1] - m[..., 1]) <= 2 * by).all()
    assert (np.abs(t[..., 2] - m[..., 2]) / z_want <= 2 * bz).all()


# ---------------------------------------------------------------------------------------------------------------------
# 8. end to end: history lands on the sheet
# ---------------------------------------------------------------------------------------------------------------------
def test_reproject_with_previous_vertices_is_the_host_rule_on_the_new_plane(instance):
    desc0 = sheet_desc()
    v0, v1 = desc0.vertices, waved(desc0.vertices, 0.2, 0.5)
    desc1 = with_vertices(desc0, v1)
    cam = desc1.camera
    ren = renderer(instance, desc1)
    ren.update_vertices(v0[N_ROOM:], first=N_ROOM)
    prev0, prev1 = ren.read_aov(0), ren.read_aov(1)
    ren.update_vertices(v1[N_ROOM:], first=N_ROOM)
    prev_color = synthetic_frame(W, H, seed=8)[0]
    prev = dict(prev_vertices=v0[N_ROOM:], first_vertex=N_ROOM)
    motion = ren.read_motion(cam, **prev)
    for params in ({}, dict(depth_tolerance=0.1)):
        out = ren.reproject(cam, prev_color, prev0, prev1, **prev, **params)
        assert np.array_equal(bits(out), bits(glaze_amd.host_reproject(motion, prev_color, prev0, prev1, **params))), params
    out = ren.reproject(cam, prev_color, prev0, prev1, **prev)
    without = ren.reproject(cam, prev_color, prev0, prev1)
    on_sheet = bits(motion[..., 3]) == SHEET
    share, share_without = (out[..., 3] > 0)[on_sheet].mean(), (without[..., 3] > 0)[on_sheet].mean()
    print("waved sheet: %.1f %% of %d sheet pixels receive history with the previous vertices, %.1f %% without" % (100 * share, on_sheet.sum(), 100 * share_without))
    assert share > share_without


# ---------------------------------------------------------------------------------------------------------------------
# 9. arguments, and nothing is disturbed
# ---------------------------------------------------------------------------------------------------------------------
def test_refused_previous_states_change_nothing(instance):
    desc0 = sheet_desc()
    desc1 = with_vertices(desc0, waved(desc0.vertices, 0.2, 0.5))
    prev_cam = moved_camera(desc1.camera)
    ren = renderer(instance, desc1)
    ren.set_seed(5)
    ren.step(3)
    hdr = ren.read_hdr()
    v0 = desc0.vertices
    n = len(v0)
    good = ren.read_motion(prev_cam, prev_vertices=v0[N_ROOM:], first_vertex=N_ROOM)
    nodes, tris = ren.scene.debug_bvh()
    two = np.stack([desc1.transforms[0]] * 2)
    refused = [read_motion_from(ren, prev_cam, vertices=v0, first=1, expect=abi.E_ARG),                   # past the vertex count
               read_motion_from(ren, prev_cam, vertices=v0[:2], first=n - 1, expect=abi.E_ARG),
               read_motion_from(ren, prev_cam, vertices=v0[:2], first=0xFFFFFFFF, expect=abi.E_ARG),      # (a sum that wraps in 32 bits)
               read_motion_from(ren, prev_cam, vertices=v0, first=0, count=0, expect=abi.E_ARG),          # none, behind a pointer that is not null
               read_motion_from(ren, prev_cam, two, v0, expect=abi.E_ARG)]                                # a transform count that is not the scene's
    for out in refused:
        assert (out == 7.0).all()                                                      # nothing was written
    # reproject_from: the same checks, and reproject's own
    frame = synthetic_frame(W, H, seed=3)
    for kw in (dict(prev_vertices=v0, first_vertex=1), dict(prev_vertices=v0[N_ROOM:], first_vertex=N_ROOM, depth_tolerance=0.0),
               dict(prev_vertices=v0[N_ROOM:], first_vertex=N_ROOM, prev_transforms=two)):
        with pytest.raises(glaze_amd.GlazeError) as e:
            ren.reproject(prev_cam, frame[0], frame[1], frame[2], **kw)
        assert e.value.status == abi.E_ARG
    with pytest.raises(glaze_amd.GlazeError) as e:
        ren.debug_motion_timing(prev_cam, prev_vertices=v0, first_vertex=1)
    assert e.value.status == abi.E_ARG
    with pytest.raises(ValueError):
        ren.read_motion(prev_cam, prev_vertices=v0["vv"])                              # positions alone are not vertices
    after = ren.scene.debug_bvh()
    assert np.array_equal(nodes, after[0]) and np.array_equal(bits(tris), bits(after[1]))
    assert np.array_equal(bits(ren.read_hdr()), bits(hdr)) and ren.stats().launches == 3
    assert np.array_equal(bits(ren.read_motion(prev_cam, prev_vertices=v0[N_ROOM:], first_vertex=N_ROOM)), bits(good))
    assert ren.debug_motion_timing(prev_cam, prev_vertices=v0[N_ROOM:], first_vertex=N_ROOM) > 0.0
    ren.set_partition(0, 2)                                                            # the full frame on this device, whatever the partition
    assert np.array_equal(bits(ren.read_motion(prev_cam, prev_vertices=v0[N_ROOM:], first_vertex=N_ROOM)), bits(good))


def test_previous_vertices_do_not_disturb_the_accumulation(instance):
    desc = atrium_scene(sponza_like=True, texture_size=64, sky_size=(64, 32))
    prev_cam = moved_camera(desc.camera, shift=(0.2, 0.05, -0.1), turn=(0.3, 0.0, 0.0))
    prev_xf = moved_transforms(desc.transforms, seed=2)
    frame = synthetic_frame(150, 83, seed=3)
    first = len(desc.vertices) // 3
    before = desc.vertices[first:].copy()
    before["vv"] += np.float32(0.05)

    def new():
        r = glaze_amd.RayTraceRenderer.new(instance, glaze_amd.RayTraceScene.from_desc(instance, desc), 150, 83)
        r.set_seed(21)
        r.set_depth(4)
        r.set_launch_mode("two_kernels")
        return r

    a, b = new(), new()
    a.step(24)
    b.step(7)
    moved = b.read_motion(prev_cam, prev_xf, prev_vertices=before, first_vertex=first)
    assert not np.array_equal(bits(moved), bits(b.read_motion(prev_cam, prev_xf)))     # the previous vertices were seen
    b.reproject(prev_cam, frame[0], frame[1], frame[2], prev_xf, prev_vertices=before, first_vertex=first)
    b.step(17)
    assert np.array_equal(bits(a.read_hdr()), bits(b.read_hdr()))
    assert np.array_equal(bits(a.read_result()), bits(b.read_result()))
    assert a.stats().launches == b.stats().launches == 24
    for which in (0, 1):
        assert np.array_equal(bits(a.read_aov(which)), bits(b.read_aov(which)))
    assert np.array_equal(bits(a.read_denoised()), bits(b.read_denoised()))
