"""Skinned meshes under a live renderer (glz_renderer_add_skin, glz_renderer_pose_skins, glz_renderer_read_vertices,
glz_renderer_read_motion_posed, glz_renderer_reproject_posed).

Two rules.  k_skin must give, bit for bit, the vertices glz_host_skin gives (tests/test_skin_host.py holds that reference to the
specification).  And a scene posed on the device must be, hit for hit and pixel for pixel, the scene test_gpu_vertex_update.py knows: one
updated with the host-skinned vertices, and one created fresh with them."""
import ctypes as C

import numpy as np
import pytest

import glaze_amd
from glaze_amd import abi
from glaze_amd.scene_desc import VERTEX_DTYPE, make_camera
from oracle.pyoracle import OracleRenderer, OracleScene

from test_gpu_motion import FOVX, moved_camera, moved_transforms
from test_gpu_vertex_update import (N_ROOM, assert_same_bytes, assert_same_hits, assert_same_render, assert_same_structure, bits, col_major, instanced_sheets,
                                    make_scene, random_transforms, render, sheet_scene, structure, waved, with_vertices)

pytestmark = pytest.mark.gpu

N_SHEET = 33 * 33
LDS_BONES = 256          # kSkinLdsBones (kernels.h): the bone table is staged in LDS up to this many bones, read from memory above


def as_rows(vertices):
    return np.ascontiguousarray(vertices).view(np.float32).reshape(-1, 8)


def as_vertices(rows):
    return np.ascontiguousarray(rows, np.float32).view(VERTEX_DTYPE).reshape(-1)


def same_finite_bits(got, want):
    fg, fw = np.isfinite(got), np.isfinite(want)
    assert np.array_equal(fg, fw)
    assert np.array_equal(got.view(np.uint32)[fg], want.view(np.uint32)[fw])


def renderer(instance, desc, levels="flat", size=(64, 48)):
    scene = make_scene(instance, desc, levels)
    return scene, glaze_amd.RayTraceRenderer.new(instance, scene, *size)


def hinge(angle, y=-0.4, z=0.55, lift=0.0):
    """a rotation about the line (x, y, z) parallel to x, then a lift along y: a rigid bone in the sheet's object space"""
    c, s = np.cos(angle), np.sin(angle)
    m = np.eye(4)
    m[1:3, 1:3] = [[c, -s], [s, c]]
    m[1:3, 3] = np.array([y, z]) - m[1:3, 1:3] @ np.array([y, z]) + (lift, 0.0)
    return col_major(m)


def bend(angle, lift=0.0):
    """two bones: the near half of the sheet stays, the far half turns about the middle line"""
    return np.stack([col_major(np.eye(4)), hinge(angle, lift=lift)])


def sheet_influences(vertices, first=N_ROOM, n=N_SHEET):
    """joints and weights of the sheet's vertices [first, first + n): bone 1 takes over smoothly across the middle third in z"""
    z = vertices["vv"][first:first + n, 2].astype(np.float64)
    s = np.clip((z - 0.4) / 0.3, 0.0, 1.0)
    w = np.stack([1.0 - s, s, np.zeros_like(s), np.zeros_like(s)], -1).astype(np.float32)
    j = np.tile(np.array([0, 1, 1, 0], np.uint16), (n, 1))
    return j, w


def host_posed(vertices, first, joints, weights, bones):
    """the whole vertex array with [first, first + n) as glz_host_skin poses it"""
    v = vertices.copy()
    n = len(joints)
    v[first:first + n] = as_vertices(glaze_amd.host_skin(vertices[first:first + n], joints, weights, bones))
    return v


# ---- 1: the kernel against the host reference ----------------------------------------------------------------------------------
def random_bones(rng, k):
    """near the identity, with scale and shear: the scene stays a scene"""
    m = np.tile(np.eye(4), (k, 1, 1))
    m[:, :3, :3] += rng.normal(size=(k, 3, 3)) * 0.15
    m[:, :3, 3] = rng.uniform(-0.1, 0.1, (k, 3))
    m[:, 3, :] = rng.normal(size=(k, 4))                                                        # the fourth row is never read
    return np.ascontiguousarray(m.transpose(0, 2, 1).reshape(k, 16), np.float32)


@pytest.mark.parametrize("n_bones", [1, 2, LDS_BONES, LDS_BONES + 1])
@pytest.mark.parametrize("first", [0, 5])
def test_kernel_equals_the_host_reference(instance, first, n_bones):
    desc = sheet_scene()
    v0 = as_rows(desc.vertices)
    scene, r = renderer(instance, desc)
    rng = np.random.default_rng(100 * first + n_bones)
    assert np.array_equal(r.read_vertices(0, len(v0)).view(np.uint32), v0.view(np.uint32))
    for n in (1, 63, 64, 65, 257):
        j = rng.integers(0, n_bones, (n, 4)).astype(np.uint16)
        j[0] = (0, n_bones - 1, n_bones - 1, 0)                                                  # bone 0 and the last one
        w = rng.normal(size=(n, 4)).astype(np.float32)                                           # negative ones, sums that are not 1
        w[rng.random((n, 4)) < 0.25] = 0.0
        bones = random_bones(rng, n_bones)
        skin = r.add_skin(first, j, w, n_bones)
        r.pose({skin: bones})
        got = r.read_vertices(0, len(v0))
        want = v0.copy()
        want[first:first + n] = glaze_amd.host_skin(v0[first:first + n], j, w, bones)
        assert not np.array_equal(want[first:first + n, :6], v0[first:first + n, :6])
        same_finite_bits(got[first:first + n], want[first:first + n])
        assert np.array_equal(got.view(np.uint32)[:first], v0.view(np.uint32)[:first])           # outside the range: untouched
        assert np.array_equal(got.view(np.uint32)[first + n:], v0.view(np.uint32)[first + n:])
        r.remove_skin(skin)
        assert np.array_equal(r.read_vertices(0, len(v0)).view(np.uint32), got.view(np.uint32))  # removing a skin leaves the vertices
        r.update_vertices(v0[first:first + n], first=first)                                       # the next skin binds the original again


def test_non_finite_bones_reach_the_vertices_the_host_says(instance):
    """a NaN and an infinity in the bones: the same vertices stop being finite on both sides (rebuild mode: the builders are the part
    of the library that is tested on such vertices, test_gpu_scene_trace.py)"""
    desc = sheet_scene()
    v0 = as_rows(desc.vertices)
    _, r = renderer(instance, desc)
    rng = np.random.default_rng(77)
    first, n, n_bones = N_ROOM + 5, 257, 4
    j = rng.integers(0, n_bones, (n, 4)).astype(np.uint16)
    j[::3] = 0                                                                                   # a third of the vertices under the finite bone alone
    w = rng.normal(size=(n, 4)).astype(np.float32)
    w[rng.random((n, 4)) < 0.25] = 0.0                                                           # 0 x inf is NaN: no term is skipped
    bones = random_bones(rng, n_bones)
    bones[1, 0], bones[2, 13], bones[3, 6] = np.nan, np.inf, -np.inf
    skin = r.add_skin(first, j, w, n_bones)
    r.pose({skin: bones}, mode="rebuild")
    got, want = r.read_vertices(first, n), glaze_amd.host_skin(v0[first:first + n], j, w, bones)
    same_finite_bits(got, want)
    assert np.isnan(got).any() and np.isinf(got).any() and np.isfinite(got[::3]).all()
    rest = r.read_vertices(0, len(v0))
    assert np.array_equal(rest.view(np.uint32)[:first], v0.view(np.uint32)[:first]) and np.array_equal(rest.view(np.uint32)[first + n:], v0.view(np.uint32)[first + n:])


# ---- 2: a posed scene is the scene created with the posed vertices ------------------------------------------------------------
def bent(instance, levels, mode, size=(64, 48), angle=0.5):
    desc = instanced_sheets(12, seed=21) if levels == "two_level" else sheet_scene()
    j, w = sheet_influences(desc.vertices)
    bones = bend(angle, lift=0.05)
    a, ra = renderer(instance, desc, levels, size)
    skin = ra.add_skin(N_ROOM, j, w, 2)
    ra.pose({skin: bones}, mode)
    return desc, host_posed(desc.vertices, N_ROOM, j, w, bones), a, ra, skin


@pytest.mark.parametrize("levels,mode", [("flat", "refit"), ("flat", "rebuild"), ("two_level", "refit")])
def test_posed_scene_equals_updated_and_fresh_scenes(instance, levels, mode):
    desc, v1, a, ra, _ = bent(instance, levels, mode)
    assert not np.array_equal(as_rows(v1)[N_ROOM:, :6], as_rows(desc.vertices)[N_ROOM:, :6])
    c, rc = renderer(instance, desc, levels)
    rc.update_vertices(v1[N_ROOM:], first=N_ROOM, mode=mode)
    assert_same_structure(a, c)
    ua, uc = ra.geometry_update_info(), rc.geometry_update_info()
    assert (ua.mode, ua.meshes_touched) == (uc.mode, uc.meshes_touched) and ua.update_ms >= 0
    assert ua.box_area == pytest.approx(uc.box_area, rel=1e-5) and ua.box_area_built == pytest.approx(uc.box_area_built, rel=1e-5)
    b, rb = renderer(instance, with_vertices(desc, v1), levels)
    assert_same_hits(a, b, 50_000)
    assert_same_render(ra, rb)
    if mode == "rebuild":
        assert_same_structure(a, b)


def test_posed_render_matches_the_oracle(instance):
    desc, v1, _, r, _ = bent(instance, "flat", "refit", size=(32, 24))
    img, _ = render(r, 5, seed=7, depth=4)
    o = OracleRenderer(OracleScene(with_vertices(desc, v1)), 32, 24)
    o.set_depth(4)
    o.set_seed(7)
    o.step(5)
    assert np.array_equal(bits(img), bits(o.read_hdr()))


# ---- 3: two skins in one call -------------------------------------------------------------------------------------------------
FIRST_A, N_A = N_ROOM, 400                     # skin A: the sheet's first 400 vertices
FIRST_B = N_ROOM + 600                         # skin B: from vertex 600 of the sheet to its end; 200 unskinned vertices between them
N_B = N_SHEET - 600


def two_skins(r, vertices):
    ja, wa = sheet_influences(vertices, FIRST_A, N_A)
    jb, wb = sheet_influences(vertices, FIRST_B, N_B)
    return (r.add_skin(FIRST_A, ja, wa, 2), ja, wa), (r.add_skin(FIRST_B, jb, wb, 2), jb, wb)


def test_two_skins_in_one_call_leave_the_gap_alone(instance):
    desc = sheet_scene()
    a, ra = renderer(instance, desc)
    (ida, ja, wa), (idb, jb, wb) = two_skins(ra, desc.vertices)
    assert ida != idb
    bones_a, bones_b = np.stack([hinge(0.0, lift=0.1), hinge(0.2)]), bend(-0.4)
    ra.pose({idb: bones_b, ida: bones_a})
    v1 = host_posed(host_posed(desc.vertices, FIRST_A, ja, wa, bones_a), FIRST_B, jb, wb, bones_b)
    got = ra.read_vertices(0, len(v1))
    same_finite_bits(got, as_rows(v1))
    gap = slice(FIRST_A + N_A, FIRST_B)
    assert np.array_equal(got[gap].view(np.uint32), as_rows(desc.vertices)[gap].view(np.uint32))
    u = ra.geometry_update_info()                                                                # ONE update of the structure
    assert (u.mode, u.meshes_touched) == (abi.GEOMETRY_REFIT, 1) and u.update_ms >= 0 and u.box_area > 0 and u.box_area_built > 0
    c, rc = renderer(instance, desc)
    rc.update_vertices(v1[N_ROOM:], first=N_ROOM)
    assert_same_structure(a, c)
    b, rb = renderer(instance, with_vertices(desc, v1))
    assert_same_hits(a, b, 50_000)
    assert_same_render(ra, rb)


# ---- 4: the host mirror -------------------------------------------------------------------------------------------------------
def test_two_level_pose_then_new_transforms_equals_a_fresh_scene(instance):
    desc, v1, a, ra, _ = bent(instance, "two_level", "refit")
    for x, y in zip(a.debug_instance_boxes(True), a.debug_instance_boxes(False)):                # the host rule reads the mirror
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    t1 = desc.transforms.copy()
    t1[1:] = random_transforms(np.random.default_rng(22), 12)
    ra.update_transforms(t1)
    both = with_vertices(desc, v1)
    both.transforms = t1
    b, rb = renderer(instance, both, "two_level")
    for x, y in zip(a.debug_instance_boxes(True), b.debug_instance_boxes(False)):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    assert_same_hits(a, b, 50_000)
    assert_same_render(ra, rb)


def test_flat_pose_then_an_update_of_other_vertices_equals_a_fresh_scene(instance):
    desc, v1, a, ra, _ = bent(instance, "flat", "refit")
    v2 = v1.copy()
    v2["vv"][:N_ROOM] *= np.float32(1.05)                                                        # the room, a little larger
    ra.update_vertices(v2[:N_ROOM], first=0)
    same_finite_bits(ra.read_vertices(0, len(v2)), as_rows(v2))
    b, rb = renderer(instance, with_vertices(desc, v2))
    assert_same_hits(a, b, 50_000)
    assert_same_render(ra, rb)
    ra.update_vertices(v2[:N_ROOM], first=0, mode="rebuild")
    assert_same_structure(a, b)


# ---- 5: the bind pose stays ---------------------------------------------------------------------------------------------------
def test_a_second_pose_starts_from_the_bind_pose(instance):
    desc, _, a, ra, skin = bent(instance, "flat", "refit")
    ra.update_vertices(waved(desc.vertices, 0.2, 0.5)[N_ROOM:], first=N_ROOM)                    # over the skinned range: allowed
    j, w = sheet_influences(desc.vertices)
    bones = bend(-0.3)
    ra.pose({skin: bones})
    v2 = host_posed(desc.vertices, N_ROOM, j, w, bones)
    same_finite_bits(ra.read_vertices(0, len(v2)), as_rows(v2))
    b, rb = renderer(instance, with_vertices(desc, v2))
    assert_same_hits(a, b, 50_000)
    assert_same_render(ra, rb)


# ---- 6: refused arguments -----------------------------------------------------------------------------------------------------
def pose_array(entries):
    """(abi.Pose array, what it points into) of (skin, bones or None, n_bones)"""
    keep = [None if b is None else np.ascontiguousarray(b, np.float32) for _, b, _ in entries]
    arr = (abi.Pose * len(entries))(*[abi.Pose(s, None if b is None else b.ctypes.data, n) for (s, _, n), b in zip(entries, keep)])
    return arr, keep


@pytest.mark.parametrize("levels", ["flat", "two_level"])
def test_refused_arguments_change_nothing(instance, levels):
    desc = instanced_sheets(10, seed=8)
    desc.camera = make_camera(position=(0, 0.35, -0.35), target=(0, -0.4, 0.55), fovx=FOVX, near=1e-3, far=100.0)
    a, r = renderer(instance, desc, levels)
    _, ref = renderer(instance, desc, levels)
    for x in (r, ref):
        x.set_depth(4)
        x.set_seed(5)
        x.step(3)
    j, w = sheet_influences(desc.vertices, N_ROOM, 500)
    skin = r.add_skin(N_ROOM, j, w, 2)                                                           # a skin that is there (binding changes no vertex)
    before, v_before = structure(a), r.read_vertices(0, len(desc.vertices))
    assert np.array_equal(v_before.view(np.uint32), as_rows(desc.vertices).view(np.uint32))
    lib, n_all = abi.lib(), len(desc.vertices)
    jp, wp = j.ctypes.data, w.ctypes.data

    def add(first, n, joints, weights, n_bones):
        s = abi.Skin(first, n, joints, weights, n_bones)
        return lib.glz_renderer_add_skin(r._h, C.cast(C.byref(s), C.c_void_p))

    far = N_ROOM + 600                                                                            # clear of the skin that is there
    assert lib.glz_renderer_add_skin(r._h, None) == abi.E_ARG
    assert add(far, 100, None, wp, 2) == abi.E_ARG and add(far, 100, jp, None, 2) == abi.E_ARG   # null pointers
    assert add(far, 0, jp, wp, 2) == abi.E_ARG                                                   # none
    assert add(n_all - 99, 100, jp, wp, 2) == abi.E_ARG and add(0xFFFFFFFF, 2, jp, wp, 2) == abi.E_ARG   # past the end (and a sum that wraps)
    assert add(far, 100, jp, wp, 0) == abi.E_ARG                                                 # no bones
    assert add(far, 100, jp, wp, 1) == abi.E_ARG                                                 # a joint >= n_bones (the joints name bone 1)
    assert add(N_ROOM + 499, 10, jp, wp, 2) == abi.E_ARG and add(0, N_ROOM + 1, jp, wp, 2) == abi.E_ARG   # overlaps, at either end
    assert lib.glz_renderer_remove_skin(r._h, skin + 1) == abi.E_ARG and lib.glz_renderer_remove_skin(r._h, -1) == abi.E_ARG
    nxt = add(far, 100, jp, wp, 2)                                                               # (and one that is fine, to name twice below)
    assert nxt == skin + 1

    two, three = bend(0.4), np.concatenate([bend(0.4), bend(0.1)[:1]])
    bad_poses = [None,                                                                            # null (and none, below)
                 [(skin + 7, two, 2)],                                                            # an unknown skin
                 [(skin, two, 2), (nxt, two, 2), (skin, two, 2)],                                 # the same skin twice
                 [(skin, three, 3)], [(skin, two, 1)],                                            # another bone count
                 [(skin, None, 2)]]                                                               # null bones
    pose = lib.glz_renderer_pose_skins
    good, keep_good = pose_array([(skin, two, 2)])
    assert pose(r._h, C.cast(good, C.c_void_p), 0, abi.GEOMETRY_REFIT) == abi.E_ARG              # none
    assert pose(r._h, C.cast(good, C.c_void_p), 1, 2) == abi.E_ARG                               # an unknown mode
    cam = moved_camera(desc.camera)
    out = np.zeros((48, 64, 4), np.float32)
    frames = [np.zeros((48, 64, 4), np.float32) for _ in range(3)]
    v_rows = as_rows(desc.vertices)

    def state(vertices=None, camera=cam):
        return abi.PreviousState(None if camera is None else C.cast(C.byref(camera), C.c_void_p), None, 0, None if vertices is None else vertices.ctypes.data, 0,
                                 0 if vertices is None else len(vertices))

    def motion_posed(st, arr, n):
        return lib.glz_renderer_read_motion_posed(r._h, None if st is None else C.cast(C.byref(st), C.c_void_p), None if arr is None else C.cast(arr, C.c_void_p), n,
                                                  out.ctypes.data)

    def reproject_posed(st, arr, n):
        return lib.glz_renderer_reproject_posed(r._h, None if st is None else C.cast(C.byref(st), C.c_void_p), None if arr is None else C.cast(arr, C.c_void_p), n,
                                                frames[0].ctypes.data, frames[1].ctypes.data, frames[2].ctypes.data, None, out.ctypes.data)

    for entries in bad_poses:
        arr, keep = (None, None) if entries is None else pose_array(entries)
        n = 1 if entries is None else len(entries)
        assert pose(r._h, None if arr is None else C.cast(arr, C.c_void_p), n, abi.GEOMETRY_REFIT) == abi.E_ARG, entries
        assert motion_posed(state(), arr, n) == abi.E_ARG and reproject_posed(state(), arr, n) == abi.E_ARG, entries
    for call in (motion_posed, reproject_posed):
        assert call(state(), good, 0) == abi.E_ARG                                               # none
        assert call(state(vertices=v_rows), good, 1) == abi.E_ARG                                # a posed state brings no vertices
        assert call(None, good, 1) == abi.E_ARG and call(state(camera=None), good, 1) == abi.E_ARG
    assert lib.glz_renderer_read_motion_posed(r._h, C.cast(C.byref(state()), C.c_void_p), C.cast(good, C.c_void_p), 1, None) == abi.E_ARG
    rv = lib.glz_renderer_read_vertices
    assert rv(r._h, 0, n_all, None) == abi.E_ARG and rv(r._h, 0, 0, out.ctypes.data) == abi.E_ARG and rv(r._h, 1, n_all, out.ctypes.data) == abi.E_ARG
    with pytest.raises(ValueError):
        r.add_skin(far + 200, j[:, :3], w[:, :3], 2)
    with pytest.raises(glaze_amd.GlazeError):
        r.pose({skin: three})

    assert_same_bytes(before, structure(a))
    assert np.array_equal(r.read_vertices(0, n_all).view(np.uint32), v_before.view(np.uint32))
    for x in (r, ref):
        x.step(4)
    assert np.array_equal(bits(r.read_hdr()), bits(ref.read_hdr()))                              # the accumulation went on, on the same scene
    assert np.array_equal(bits(r.read_result()), bits(ref.read_result()))


# ---- 7: the other devices of set_devices --------------------------------------------------------------------------------------
@pytest.fixture
def loopback(monkeypatch):
    monkeypatch.setenv("GLAZE_MULTI_LOOPBACK", "1")


@pytest.mark.parametrize("levels", ["flat", "two_level"])
@pytest.mark.parametrize("devices_first", [True, False])
def test_loopback_devices_follow_a_pose(instance, loopback, levels, devices_first):
    desc = instanced_sheets(10, seed=9)
    j, w = sheet_influences(desc.vertices)
    bones = bend(0.45)
    r = glaze_amd.RayTraceRenderer.new(instance, make_scene(instance, desc, levels), 136, 200)
    if devices_first:
        r.set_devices([instance.device] * 2)
    skin = r.add_skin(N_ROOM, j, w, 2)
    r.pose({skin: bend(-0.2)})
    if not devices_first:
        r.set_devices([instance.device] * 2)                                                     # the replica is made of the posed scene, skins included
    r.pose({skin: bones})
    one = glaze_amd.RayTraceRenderer.new(instance, make_scene(instance, with_vertices(desc, host_posed(desc.vertices, N_ROOM, j, w, bones)), levels), 136, 200)
    assert_same_render(r, one)
    assert np.array_equal(r.read_rgba8(), one.read_rgba8())


# ---- 8: motion and reprojection that follow a pose ----------------------------------------------------------------------------
@pytest.mark.parametrize("levels", ["flat", "two_level"])
@pytest.mark.parametrize("with_transforms", [False, True])
def test_posed_motion_and_reprojection_equal_the_host_skinned_ones(instance, levels, with_transforms):
    desc = instanced_sheets(10, seed=31) if levels == "two_level" else sheet_scene()
    desc.camera = make_camera(position=(0, 0.35, -0.35), target=(0, -0.4, 0.55), fovx=FOVX, near=1e-3, far=100.0)
    _, r = renderer(instance, desc, levels)
    (ida, ja, wa), (idb, jb, wb) = two_skins(r, desc.vertices)
    now = {ida: np.stack([hinge(0.0, lift=0.05), hinge(0.3)]), idb: bend(0.4)}
    before = {ida: np.stack([hinge(0.0), hinge(0.1)]), idb: bend(0.1, lift=0.05)}
    r.pose(now)
    cam = moved_camera(desc.camera, shift=(0.1, 0.05, -0.1), turn=(0.1, -0.05, 0.1))
    t0 = moved_transforms(desc.transforms, 5) if with_transforms else None
    # the previous vertices over the posed span, on the host: the current ones (the gap keeps them), then each skin as its previous bones pose it
    bind = desc.vertices
    span = as_vertices(r.read_vertices(FIRST_A, N_SHEET))
    span[:N_A] = as_vertices(glaze_amd.host_skin(bind[FIRST_A:FIRST_A + N_A], ja, wa, before[ida]))
    span[FIRST_B - FIRST_A:] = as_vertices(glaze_amd.host_skin(bind[FIRST_B:FIRST_B + N_B], jb, wb, before[idb]))
    want = r.read_motion(cam, t0, prev_vertices=span, first_vertex=FIRST_A)
    got = r.read_motion(cam, t0, prev_poses=before)
    assert np.array_equal(bits(got), bits(want))
    if levels == "flat":                                                                         # (the camera looks at the sheet there)
        assert not np.array_equal(bits(got), bits(r.read_motion(cam, t0)))                       # the pose did move what it sees
    one = r.read_motion(cam, t0, prev_poses={idb: before[idb]})                                  # one skin: its own span
    span_b = as_vertices(glaze_amd.host_skin(bind[FIRST_B:FIRST_B + N_B], jb, wb, before[idb]))
    assert np.array_equal(bits(one), bits(r.read_motion(cam, t0, prev_vertices=span_b, first_vertex=FIRST_B)))
    rng = np.random.default_rng(3)
    color = rng.random((48, 64, 4)).astype(np.float32)
    aov0, aov1 = r.read_aov(0), r.read_aov(1)
    for params in ({}, dict(depth_tolerance=0.5)):
        got = r.reproject(cam, color, aov0, aov1, t0, prev_poses=before, **params)
        want = r.reproject(cam, color, aov0, aov1, t0, prev_vertices=span, first_vertex=FIRST_A, **params)
        assert np.array_equal(bits(got), bits(want))
        if levels == "flat" and not with_transforms and params:
            assert (got[..., 3] > 0).any()                                                       # (and it is no empty frame that agrees)


# ---- 9: whoever holds the scene sees skins and poses --------------------------------------------------------------------------
# (Two renderers on one scene cannot be had through the C interface -- glz_renderer_create takes the scene over and refuses one that
# belongs to a renderer, see test_gpu_vertex_update.py -- so the second holder here is the scene handle, as in every case above that
# traces A through it: the skin is added and posed through the renderer and lives in the scene, which outlives the renderer.)
def test_the_scene_handle_sees_skins_and_poses(instance):
    desc, v1, a, ra, skin = bent(instance, "flat", "refit")
    b = make_scene(instance, with_vertices(desc, v1))
    assert_same_hits(a, b, 20_000)
    del ra                                                                                        # the scene, its skin and its pose stay
    assert_same_hits(a, b, 20_000, seed=1)
