"""Skins in dual-quaternion mode under a live renderer (glz_renderer_set_skin_blend, glz_renderer_skin_blend; k_skin_dq, k_morph_skin_dq).

The two rules of test_gpu_skin.py, for the mode: the kernels must give, bit for bit, the vertices glz_host_skin_dq gives
(tests/test_skin_dq_host.py holds that reference to the specification), and a scene posed on the device must be, hit for hit and pixel for
pixel, one updated with the host-skinned vertices and one created fresh with them.  The linear mode is what it was: a skin switched back
gives glz_host_skin again."""
import numpy as np
import pytest

import glaze_amd
from glaze_amd import abi
from glaze_amd.scene_desc import make_camera

import test_gpu_morph as gm
from test_gpu_morph import LDS_TARGETS, same_bits
from test_gpu_motion import FOVX, moved_camera
from test_gpu_skin import (FIRST_A, FIRST_B, LDS_BONES, N_A, N_B, N_SHEET, as_rows, as_vertices, bend, hinge, loopback, random_bones, renderer,  # noqa: F401
                           same_finite_bits, sheet_influences)
from test_gpu_vertex_update import (N_ROOM, assert_same_bytes, assert_same_hits, assert_same_render, assert_same_structure, bits, col_major, instanced_sheets,
                                    make_scene, sheet_scene, structure, with_vertices)
from test_morph_host import random_targets, random_weights
from test_skin_dq_host import about_x, turned_bones

pytestmark = pytest.mark.gpu

DQ = "dual_quaternion"


def host_skin_dq(bind, joints, weights, bones):
    return glaze_amd.host_skin(bind, joints, weights, bones, blend=DQ)


def host_posed(vertices, first, joints, weights, bones, blend=DQ):
    """the whole vertex array with [first, first + n) as the host reference of `blend` poses it"""
    v = vertices.copy()
    n = len(joints)
    v[first:first + n] = as_vertices(glaze_amd.host_skin(vertices[first:first + n], joints, weights, bones, blend=blend))
    return v


def mixed_bones(rng, k):
    """rigid bones over all rotations (every Shepperd branch, test_skin_dq_host.py), every third one with scale and shear instead, and the
    +100 / -100 degree pair, whose second weight the sign step negates, as bone 0 and the last one"""
    bones = turned_bones(rng, k, reach=0.3)
    bones[2::3] = random_bones(rng, k)[2::3]
    if k >= 2:
        bones[0], bones[-1] = col_major(about_x(np.radians(100.0))), col_major(about_x(np.radians(-100.0)))
    return bones


def mixed_influences(rng, n, k):
    j = rng.integers(0, k, (n, 4)).astype(np.uint16)
    j[0] = (0, k - 1, k - 1, 0)                                                                  # bone 0 and the last one: the +-100 degree pair
    w = rng.normal(size=(n, 4)).astype(np.float32)                                               # negative ones, sums that are not 1
    w[rng.random((n, 4)) < 0.25] = 0.0
    w[(w == 0).all(1), 0] = 1.0                                                                  # (a blend of nothing is not finite: the last test's)
    w[0] = (0.5, 0.25, 0.25, 0.0)
    return j, w


# ---- 1: the kernel against the host reference ----------------------------------------------------------------------------------
@pytest.mark.parametrize("n_bones", [1, 2, LDS_BONES, LDS_BONES + 1])
@pytest.mark.parametrize("first", [0, 5])
def test_kernel_equals_the_host_reference(instance, first, n_bones):
    desc = sheet_scene()
    v0 = as_rows(desc.vertices)
    scene, r = renderer(instance, desc)
    rng = np.random.default_rng(100 * first + n_bones)
    for n in (1, 63, 64, 65, 257):
        j, w = mixed_influences(rng, n, n_bones)
        bones = mixed_bones(rng, n_bones)
        skin = r.add_skin(first, j, w, n_bones, blend=DQ)
        assert r.skin_blend(skin) == DQ
        r.pose({skin: bones})
        got = r.read_vertices(0, len(v0))
        want = host_skin_dq(v0[first:first + n], j, w, bones)
        assert np.isfinite(want).all() and not np.array_equal(want[:, :6], v0[first:first + n, :6])
        assert not np.array_equal(want, glaze_amd.host_skin(v0[first:first + n], j, w, bones))   # (the other rule gives other vertices)
        same_finite_bits(got[first:first + n], want)
        assert same_bits(got[:first], v0[:first]) and same_bits(got[first + n:], v0[first + n:])  # outside the range: untouched
        r.remove_skin(skin)
        assert same_bits(r.read_vertices(0, len(v0)), got)                                        # removing a skin leaves the vertices
        r.update_vertices(v0[first:first + n], first=first)                                       # the next skin binds the original again


# ---- 2: the mode is the skin's, and switches ----------------------------------------------------------------------------------------
def test_a_skin_switches_between_the_rules_and_bad_arguments_change_nothing(instance):
    desc = sheet_scene()
    v0 = as_rows(desc.vertices)
    a, r = renderer(instance, desc)
    j, w = sheet_influences(desc.vertices)
    bones = bend(0.9, lift=0.05)
    bind = v0[N_ROOM:N_ROOM + N_SHEET]
    want_lin, want_dq = glaze_amd.host_skin(bind, j, w, bones), host_skin_dq(bind, j, w, bones)
    assert not np.array_equal(want_lin, want_dq)
    skin = r.add_skin(N_ROOM, j, w, 2)
    assert r.skin_blend(skin) == "linear"
    r.pose({skin: bones})
    same_finite_bits(r.read_vertices(N_ROOM, N_SHEET), want_lin)
    before = structure(a)
    r.set_skin_blend(skin, DQ)
    assert r.skin_blend(skin) == DQ
    assert same_bits(r.read_vertices(N_ROOM, N_SHEET), want_lin)                                 # setting the mode writes no vertex
    assert_same_bytes(before, structure(a))
    lib = abi.lib()
    for bad_skin, bad_mode in ((skin + 1, abi.SKIN_LINEAR), (-1, abi.SKIN_LINEAR), (skin, 2), (skin, -1)):
        assert lib.glz_renderer_set_skin_blend(r._h, bad_skin, bad_mode) == abi.E_ARG
    assert lib.glz_renderer_skin_blend(r._h, skin + 1) == abi.E_ARG and lib.glz_renderer_skin_blend(r._h, -1) == abi.E_ARG
    with pytest.raises(ValueError):
        r.set_skin_blend(skin, "quaternion")
    assert r.skin_blend(skin) == DQ                                                              # ... and changed nothing
    r.pose({skin: bones})
    same_finite_bits(r.read_vertices(N_ROOM, N_SHEET), want_dq)
    r.set_skin_blend(skin, "linear")
    assert r.skin_blend(skin) == "linear"
    r.pose({skin: bones})
    same_finite_bits(r.read_vertices(N_ROOM, N_SHEET), want_lin)
    assert same_bits(r.read_vertices(0, N_ROOM), v0[:N_ROOM])


# ---- 3: a posed scene is the scene created with the posed vertices ------------------------------------------------------------
@pytest.mark.parametrize("levels,mode", [("flat", "refit"), ("flat", "rebuild"), ("two_level", "refit")])
def test_posed_scene_equals_updated_and_fresh_scenes(instance, levels, mode):
    desc = instanced_sheets(12, seed=21) if levels == "two_level" else sheet_scene()
    j, w = sheet_influences(desc.vertices)
    bones = bend(0.5, lift=0.05)
    a, ra = renderer(instance, desc, levels)
    skin = ra.add_skin(N_ROOM, j, w, 2, blend=DQ)
    ra.pose({skin: bones}, mode)
    v1 = host_posed(desc.vertices, N_ROOM, j, w, bones)
    assert not np.array_equal(as_rows(v1)[N_ROOM:, :6], as_rows(desc.vertices)[N_ROOM:, :6])
    same_finite_bits(ra.read_vertices(0, len(v1)), as_rows(v1))
    c, rc = renderer(instance, desc, levels)
    rc.update_vertices(v1[N_ROOM:], first=N_ROOM, mode=mode)
    assert_same_structure(a, c)
    b, rb = renderer(instance, with_vertices(desc, v1), levels)
    assert_same_hits(a, b, 50_000)
    assert_same_render(ra, rb)
    if mode == "rebuild":
        assert_same_structure(a, b)


# ---- 4: the fused kernel ------------------------------------------------------------------------------------------------------
def tiny_targets(rng, n, n_targets):
    """a few targets of a few entries; of many targets all but the first, the last and one in the middle are empty"""
    some = {0, n_targets // 2, n_targets - 1} if n_targets > 8 else set(range(n_targets))
    return random_targets(rng, n, n_targets, min(n, 5), empty=set(range(n_targets)) - some)


@pytest.mark.parametrize("n_bones", [LDS_BONES, LDS_BONES + 1])
@pytest.mark.parametrize("n_targets", [3, LDS_TARGETS, LDS_TARGETS + 1])
def test_fused_kernel_equals_skin_of_morph(instance, n_targets, n_bones):
    desc = sheet_scene()
    v0 = as_rows(desc.vertices)
    _, r = renderer(instance, desc)
    rng = np.random.default_rng(n_targets + 7 * n_bones)
    first = 5
    for n in (1, 65, 257):
        j, sw = mixed_influences(rng, n, n_bones)
        bones = mixed_bones(rng, n_bones)
        targets = tiny_targets(rng, n, n_targets)
        w = random_weights(rng, n_targets)
        w[[0, n_targets // 2, n_targets - 1]] = (0.75, -1.5, 2.0)
        skin = r.add_skin(first, j, sw, n_bones, blend=DQ)
        morph = r.add_morph(first, targets, skin=skin)
        r.animate(morphs={morph: w}, poses={skin: bones})
        got = r.read_vertices(0, len(v0))
        want = host_skin_dq(glaze_amd.host_morph(v0[first:first + n], targets, w), j, sw, bones)
        assert not np.array_equal(want[:, :6], host_skin_dq(v0[first:first + n], j, sw, bones)[:, :6])
        same_finite_bits(got[first:first + n], want)
        assert same_bits(got[:first], v0[:first]) and same_bits(got[first + n:], v0[first + n:])
        r.pose({skin: bones})                                                                     # the pose alone ignores the morph: k_skin_dq
        same_finite_bits(r.read_vertices(first, n), host_skin_dq(v0[first:first + n], j, sw, bones))
        r.remove_morph(morph)
        r.remove_skin(skin)
        r.update_vertices(v0[first:first + n], first=first)


# ---- 5: motion and reprojection that follow a pose ----------------------------------------------------------------------------
@pytest.mark.parametrize("levels", ["flat", "two_level"])
def test_posed_motion_and_reprojection_equal_the_host_skinned_ones(instance, levels):
    """two skins in one call, A in dual-quaternion mode and B linear: the previous-pose pass follows each skin's mode"""
    desc = instanced_sheets(10, seed=31) if levels == "two_level" else sheet_scene()
    desc.camera = make_camera(position=(0, 0.35, -0.35), target=(0, -0.4, 0.55), fovx=FOVX, near=1e-3, far=100.0)
    _, r = renderer(instance, desc, levels)
    ja, wa = sheet_influences(desc.vertices, FIRST_A, N_A)
    jb, wb = sheet_influences(desc.vertices, FIRST_B, N_B)
    ida, idb = r.add_skin(FIRST_A, ja, wa, 2, blend=DQ), r.add_skin(FIRST_B, jb, wb, 2)
    now = {ida: np.stack([hinge(0.1, lift=0.05), hinge(0.6)]), idb: bend(0.4)}
    before = {ida: np.stack([hinge(0.15, lift=0.02), hinge(0.45)]), idb: bend(0.1, lift=0.05)}   # (no identity: both of A's bones turn)
    r.pose(now)
    cam = moved_camera(desc.camera, shift=(0.1, 0.05, -0.1), turn=(0.1, -0.05, 0.1))
    bind = desc.vertices
    span = as_vertices(r.read_vertices(FIRST_A, N_SHEET))
    prev_a = host_skin_dq(bind[FIRST_A:FIRST_A + N_A], ja, wa, before[ida])
    assert not np.array_equal(prev_a, glaze_amd.host_skin(bind[FIRST_A:FIRST_A + N_A], ja, wa, before[ida]))
    span[:N_A] = as_vertices(prev_a)
    span[FIRST_B - FIRST_A:] = as_vertices(glaze_amd.host_skin(bind[FIRST_B:FIRST_B + N_B], jb, wb, before[idb]))
    want = r.read_motion(cam, None, prev_vertices=span, first_vertex=FIRST_A)
    got = r.read_motion(cam, None, prev_poses=before)
    assert np.array_equal(bits(got), bits(want))
    if levels == "flat":                                                                         # (the camera looks at the sheet there)
        assert not np.array_equal(bits(got), bits(r.read_motion(cam, None)))                     # the pose did move what it sees
    one = r.read_motion(cam, None, prev_poses={ida: before[ida]})                                # the dual-quaternion skin alone: its own span
    assert np.array_equal(bits(one), bits(r.read_motion(cam, None, prev_vertices=as_vertices(prev_a), first_vertex=FIRST_A)))
    rng = np.random.default_rng(3)
    color = rng.random((48, 64, 4)).astype(np.float32)
    aov0, aov1 = r.read_aov(0), r.read_aov(1)
    got = r.reproject(cam, color, aov0, aov1, None, prev_poses=before, depth_tolerance=0.5)
    want = r.reproject(cam, color, aov0, aov1, None, prev_vertices=span, first_vertex=FIRST_A, depth_tolerance=0.5)
    assert np.array_equal(bits(got), bits(want))
    if levels == "flat":
        assert (got[..., 3] > 0).any()                                                           # (and it is no empty frame that agrees)


# ---- 6: the other devices of set_devices --------------------------------------------------------------------------------------
@pytest.mark.parametrize("levels,devices_first", [("flat", True), ("flat", False), ("two_level", False)])
def test_loopback_devices_follow_the_mode(instance, loopback, levels, devices_first):
    """the mode set after the devices are attached is forwarded to them; set before, the replica made later has it.  The replica renders
    half of the frame's tiles from its own vertices, so the frame is what tells on them."""
    desc = instanced_sheets(10, seed=9)
    j, w = sheet_influences(desc.vertices)
    bones = bend(0.9)
    r = glaze_amd.RayTraceRenderer.new(instance, make_scene(instance, desc, levels), 136, 200)
    if devices_first:
        r.set_devices([instance.device] * 2)
    skin = r.add_skin(N_ROOM, j, w, 2)
    r.pose({skin: bend(-0.2)})
    r.set_skin_blend(skin, DQ)
    if not devices_first:
        r.set_devices([instance.device] * 2)                                                     # the replica is made of the posed scene, skins and modes included
    assert r.skin_blend(skin) == DQ
    r.pose({skin: bones})
    v1 = host_posed(desc.vertices, N_ROOM, j, w, bones)
    assert not np.array_equal(as_rows(v1), as_rows(host_posed(desc.vertices, N_ROOM, j, w, bones, blend="linear")))
    same_finite_bits(r.read_vertices(0, len(v1)), as_rows(v1))
    one = glaze_amd.RayTraceRenderer.new(instance, make_scene(instance, with_vertices(desc, v1), levels), 136, 200)
    assert_same_render(r, one)
    assert np.array_equal(r.read_rgba8(), one.read_rgba8())


# ---- 7: bones that are not finite ---------------------------------------------------------------------------------------------
def test_non_finite_bones_reach_the_vertices_the_host_says(instance):
    """a NaN and an infinity in the bones, and a blend of nothing (weights 1, -1 on one bone): the same vertices stop being finite on both
    sides (rebuild mode, as in test_gpu_skin.py)"""
    desc = sheet_scene()
    v0 = as_rows(desc.vertices)
    _, r = renderer(instance, desc)
    rng = np.random.default_rng(77)
    first, n, n_bones = N_ROOM + 5, 257, 4
    j = rng.integers(0, n_bones, (n, 4)).astype(np.uint16)
    j[::3] = 0                                                                                   # a third of the vertices under the finite bone alone
    w = rng.normal(size=(n, 4)).astype(np.float32)
    w[rng.random((n, 4)) < 0.25] = 0.0
    w[::3, 0] = 1.5
    j[3], w[3] = 0, (1.0, -1.0, 0.0, 0.0)                                                        # nn = 0
    bones = random_bones(rng, n_bones)
    bones[1, 0], bones[2, 13], bones[3, 6] = np.nan, np.inf, -np.inf
    skin = r.add_skin(first, j, w, n_bones, blend=DQ)
    r.pose({skin: bones}, mode="rebuild")
    got, want = r.read_vertices(first, n), host_skin_dq(v0[first:first + n], j, w, bones)
    same_finite_bits(got, want)
    rest = np.ones(n, bool)
    rest[3] = False
    assert not np.isfinite(got[3, :6]).any() and np.isfinite(got[::3][rest[::3]]).all()
    assert (~np.isfinite(got[rest])).any()
    whole = r.read_vertices(0, len(v0))
    assert same_bits(whole[:first], v0[:first]) and same_bits(whole[first + n:], v0[first + n:])


# ---- 8: two rules in one call -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("blend_b,blend_c", [(DQ, "linear"), ("linear", DQ)])
def test_one_call_runs_each_skin_by_its_own_rule(instance, blend_b, blend_c):
    """a free-standing morph, a morphed skin (B) and a plain skin (C) named in one animate (three_parts of test_gpu_morph.py), the two skins
    in different modes: every part is the host morph followed by the host skin of its own skin's mode, and the gaps keep their bits"""
    desc = sheet_scene()
    v0 = as_rows(desc.vertices)
    _, r = renderer(instance, desc)
    (ma, ta), (sb, jb, swb, mb, tb), (sc, jc, swc) = gm.three_parts(r, desc.vertices)
    r.set_skin_blend(sb, blend_b)
    r.set_skin_blend(sc, blend_c)
    wa, wb = np.array([1.0, -0.5], np.float32), np.array([0.5, 1.5, 3.0], np.float32)
    bones_b, bones_c = np.stack([hinge(0.3, lift=0.05), hinge(0.8)]), bend(-0.6)
    r.animate(morphs={mb: wb, ma: wa}, poses={sc: bones_c, sb: bones_b})

    def host(rule_b, rule_c):
        v = gm.host_morphed(desc.vertices, gm.FIRST_A, gm.N_A, ta, wa)
        v = host_posed(gm.host_morphed(v, gm.FIRST_B, gm.N_B, tb, wb), gm.FIRST_B, jb, swb, bones_b, blend=rule_b)
        return as_rows(host_posed(v, gm.FIRST_C, jc, swc, bones_c, blend=rule_c))

    want, swapped = host(blend_b, blend_c), host(blend_c, blend_b)
    part_b, part_c = slice(gm.FIRST_B, gm.FIRST_B + gm.N_B), slice(gm.FIRST_C, gm.FIRST_C + gm.N_C)
    assert not np.array_equal(want[part_b], swapped[part_b]) and not np.array_equal(want[part_c], swapped[part_c])   # (either rule swapped would show)
    got = r.read_vertices(0, len(v0))
    same_finite_bits(got, want)
    for gap in (slice(0, gm.FIRST_A), slice(gm.FIRST_A + gm.N_A, gm.FIRST_B), slice(gm.FIRST_B + gm.N_B, gm.FIRST_C)):
        assert same_bits(got[gap], v0[gap])
    for part in (slice(gm.FIRST_A, gm.FIRST_A + gm.N_A), part_b, part_c):
        assert not np.array_equal(got[part, :6], v0[part, :6])
