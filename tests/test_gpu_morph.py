"""Morph targets under a live renderer (glz_renderer_add_morph, glz_renderer_animate, glz_renderer_read_motion_animated,
glz_renderer_reproject_animated).

Two rules, as for skins.  k_morph must give, bit for bit, the vertices glz_host_morph gives, and k_morph_skin those of glz_host_skin on
them (tests/test_morph_host.py and tests/test_skin_host.py hold the references to the specification).  And a scene animated on the device
must be, hit for hit and pixel for pixel, the scene test_gpu_vertex_update.py knows: one updated with the host-made vertices, and one
created fresh with them."""
import ctypes as C

import numpy as np
import pytest

import glaze_amd
from glaze_amd import abi
from glaze_amd.scene_desc import make_camera
from oracle.pyoracle import OracleRenderer, OracleScene

from test_gpu_motion import FOVX, moved_camera, moved_transforms
from test_gpu_skin import (LDS_BONES, N_SHEET, as_rows, as_vertices, bend, hinge, host_posed, loopback, pose_array, random_bones, renderer,  # noqa: F401
                           same_finite_bits, sheet_influences)
from test_gpu_vertex_update import (N_ROOM, assert_same_bytes, assert_same_hits, assert_same_render, assert_same_structure, bits, instanced_sheets, make_scene, render,
                                    sheet_scene, structure, with_vertices)
from test_morph_host import random_target, random_targets, random_weights, target_array

pytestmark = pytest.mark.gpu

LDS_TARGETS = abi.MORPH_LDS_TARGETS     # kMorphLdsTargets (kernels.h): the weight table is staged in LDS up to this many targets, read from memory above


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def host_morphed(vertices, first, n, targets, weights):
    """the whole vertex array with [first, first + n) as glz_host_morph makes it"""
    v = vertices.copy()
    v[first:first + n] = as_vertices(glaze_amd.host_morph(vertices[first:first + n], targets, weights))
    return v


# ---- 1: the kernel against the host reference ----------------------------------------------------------------------------------
def built_targets(rng, n, n_targets, variant):
    """random sparse targets of about n / 8 entries each, and in them what the layout can get wrong.  "dense": target 0 has no index list.
    "rows": vertex 0's row is empty and vertex 1, in the same slice, is in every target; from 65 vertices on the second slice is wholly
    empty, and at 257 the third slice's only entries belong to its last lane (vertex 191)."""
    per = max(1, n // 8)
    targets = random_targets(rng, n, n_targets, per, dense=(0,) if variant == "dense" else ())
    if variant == "dense" or n < 2:
        return targets
    out = []
    for idx, dp, dn in targets:
        keep = (idx != 0) & (idx != 1) & ((idx < 64) | (idx >= 128)) & ((idx < 128) | (idx >= 192))
        idx = np.concatenate([[1], idx[keep], [191] if n > 191 else []]).astype(np.uint32)
        idx.sort()
        d = (rng.normal(size=(2, len(idx), 3)) * 0.1).astype(np.float32)
        out.append((idx, d[0], d[1]))
    return out


@pytest.mark.parametrize("n_targets", [1, 2, LDS_TARGETS, LDS_TARGETS + 1])
@pytest.mark.parametrize("first", [0, 5])
def test_kernel_equals_the_host_reference(instance, first, n_targets):
    desc = sheet_scene()
    v0 = as_rows(desc.vertices)
    scene, r = renderer(instance, desc)
    rng = np.random.default_rng(100 * first + n_targets)
    ids = []
    for n in (1, 63, 64, 65, 257):
        for variant in ("dense", "rows"):
            targets = built_targets(rng, n, n_targets, variant)
            w = random_weights(rng, n_targets)
            w[0] = 0.5
            morph = r.add_morph(first, targets, n_vertices=n)
            ids.append(morph)
            r.animate(morphs={morph: w})
            got = r.read_vertices(0, len(v0))
            want = v0.copy()
            want[first:first + n] = glaze_amd.host_morph(v0[first:first + n], targets, w)
            assert not np.array_equal(want[first:first + n, :6], v0[first:first + n, :6])
            same_finite_bits(got[first:first + n], want[first:first + n])
            assert same_bits(got[:first], v0[:first]) and same_bits(got[first + n:], v0[first + n:])     # outside the range: untouched
            if variant == "rows" and n >= 2:
                assert same_bits(got[first], v0[first])                                                   # the empty row: the bits it went in with
            r.remove_morph(morph)
            assert same_bits(r.read_vertices(0, len(v0)), got)                                            # removing a morph leaves the vertices
            r.update_vertices(v0[first:first + n], first=first)                                           # the next morph's base is the original again
    assert ids == list(range(len(ids)))                                                                   # ids count up and are never reused


def test_non_finite_weights_and_deltas_reach_the_vertices_the_host_says(instance):
    """rebuild mode, as the skin test: the builders are the part of the library that is tested on such vertices"""
    desc = sheet_scene()
    v0 = as_rows(desc.vertices)
    _, r = renderer(instance, desc)
    rng = np.random.default_rng(77)
    first, n = N_ROOM + 5, 257
    targets = []
    for t in range(5):
        idx, dp, dn = random_target(rng, n, 60 if t < 4 else 6)                                          # (few under the NaN weight: it leaves nothing else to see)
        keep = idx % 3 != 0                                                                               # a third of the vertices stay untouched
        targets.append((idx[keep], dp[keep], dn[keep]))
    targets[1][1][0, 0], targets[2][2][1, 1], targets[3][1][2, 2] = np.inf, -np.inf, np.nan
    w = np.array([0.5, 0.0, -1.0, 2.0, np.nan], np.float32)                                              # 0 x inf is NaN: no term is skipped
    morph = r.add_morph(first, targets, n_vertices=n)
    r.animate(morphs={morph: w}, mode="rebuild")
    got, want = r.read_vertices(first, n), glaze_amd.host_morph(v0[first:first + n], targets, w)
    same_finite_bits(got, want)
    assert np.isnan(got).any() and np.isinf(got).any() and np.isfinite(got[::3]).all()
    assert np.isnan(got[targets[1][0][0], 0])
    rest = r.read_vertices(0, len(v0))
    assert same_bits(rest[:first], v0[:first]) and same_bits(rest[first + n:], v0[first + n:])


# ---- 2: a morphed scene is the scene created with the morphed vertices ---------------------------------------------------------
def sheet_targets(vertices, first=N_ROOM, n=N_SHEET):
    """three targets over the sheet's vertices [first, first + n) that keep the scene a scene: a dense bulge, a sparse lift of the far
    half, and every third vertex with a tilted normal"""
    p = vertices["vv"][first:first + n].astype(np.float64)
    c = 0.5 * (p.min(0) + p.max(0))
    bulge = 0.15 * np.exp(-((p[:, 0] - c[0]) ** 2 + (p[:, 2] - c[2]) ** 2) / 0.05)
    dense = (None, np.stack([0 * bulge, bulge, 0 * bulge], -1).astype(np.float32), np.stack([0.3 * (p[:, 0] - c[0]), 0 * bulge, 0.3 * (p[:, 2] - c[2])], -1).astype(np.float32))
    far = np.nonzero(p[:, 2] > c[2])[0].astype(np.uint32)
    lift = (far, np.stack([0 * far, 0.2 * (p[far, 2] - c[2]), 0.02 + 0 * far], -1).astype(np.float32), np.zeros((len(far), 3), np.float32))
    third = np.arange(0, n, 3, dtype=np.uint32)
    tilt = (third, np.full((len(third), 3), 0.002, np.float32), np.tile(np.array([0.1, 0.0, -0.1], np.float32), (len(third), 1)))
    return [dense, lift, tilt]


WEIGHTS = np.array([0.8, -0.5, 1.0], np.float32)


def morphed(instance, levels, mode, size=(64, 48), weights=WEIGHTS):
    desc = instanced_sheets(12, seed=21) if levels == "two_level" else sheet_scene()
    targets = sheet_targets(desc.vertices)
    a, ra = renderer(instance, desc, levels, size)
    morph = ra.add_morph(N_ROOM, targets)
    ra.animate(morphs={morph: weights}, mode=mode)
    return desc, host_morphed(desc.vertices, N_ROOM, N_SHEET, targets, weights), a, ra, morph


@pytest.mark.parametrize("levels,mode", [("flat", "refit"), ("flat", "rebuild"), ("two_level", "refit")])
def test_morphed_scene_equals_updated_and_fresh_scenes(instance, levels, mode):
    desc, v1, a, ra, _ = morphed(instance, levels, mode)
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


def test_morphed_render_matches_the_oracle(instance):
    desc, v1, _, r, _ = morphed(instance, "flat", "refit", size=(32, 24))
    img, _ = render(r, 5, seed=7, depth=4)
    o = OracleRenderer(OracleScene(with_vertices(desc, v1)), 32, 24)
    o.set_depth(4)
    o.set_seed(7)
    o.step(5)
    assert np.array_equal(bits(img), bits(o.read_hdr()))


# ---- 3: the fused kernel ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_bones", [LDS_BONES, LDS_BONES + 1])
@pytest.mark.parametrize("n_targets", [LDS_TARGETS, LDS_TARGETS + 1])
def test_fused_kernel_equals_skin_of_morph(instance, n_targets, n_bones):
    desc = sheet_scene()
    v0 = as_rows(desc.vertices)
    _, r = renderer(instance, desc)
    rng = np.random.default_rng(n_targets + 7 * n_bones)
    first = 5
    for n in (1, 64, 65, 257):
        j = rng.integers(0, n_bones, (n, 4)).astype(np.uint16)
        j[0] = (0, n_bones - 1, n_bones - 1, 0)
        sw = rng.normal(size=(n, 4)).astype(np.float32)
        bones = random_bones(rng, n_bones)
        targets = built_targets(rng, n, n_targets, "rows" if n > 1 else "dense")
        w = random_weights(rng, n_targets)
        skin = r.add_skin(first, j, sw, n_bones)
        morph = r.add_morph(first, targets, skin=skin)
        r.animate(morphs={morph: w}, poses={skin: bones})
        got = r.read_vertices(0, len(v0))
        between = glaze_amd.host_morph(v0[first:first + n], targets, w)
        want = glaze_amd.host_skin(between, j, sw, bones)
        assert not np.array_equal(want[:, :6], glaze_amd.host_skin(v0[first:first + n], j, sw, bones)[:, :6])
        same_finite_bits(got[first:first + n], want)
        assert same_bits(got[:first], v0[:first]) and same_bits(got[first + n:], v0[first + n:])
        r.remove_morph(morph)
        r.remove_skin(skin)
        r.update_vertices(v0[first:first + n], first=first)


@pytest.mark.parametrize("attached", [False, True])
def test_slices_without_padding_equal_the_host_reference(instance, attached):
    """only dense targets: every row is as long as its slice is wide, which the kernels run without a lane mask (kernels_deform.hip);
    at 65 and 257 vertices the last slice holds one lane, at 63 none is full"""
    desc = sheet_scene()
    v0 = as_rows(desc.vertices)
    _, r = renderer(instance, desc)
    rng = np.random.default_rng(9 + attached)
    first, n_bones = N_ROOM + 3, 5
    for n in (1, 63, 65, 257):
        targets = random_targets(rng, n, 6, None, dense=range(6))
        w = random_weights(rng, 6)
        w[0] = 0.5
        want = glaze_amd.host_morph(v0[first:first + n], targets, w)
        if attached:
            j, sw, bones = rng.integers(0, n_bones, (n, 4)).astype(np.uint16), rng.normal(size=(n, 4)).astype(np.float32), random_bones(rng, n_bones)
            skin = r.add_skin(first, j, sw, n_bones)
            morph = r.add_morph(first, targets, skin=skin)
            r.animate(morphs={morph: w}, poses={skin: bones})
            want = glaze_amd.host_skin(want, j, sw, bones)
        else:
            morph = r.add_morph(first, targets)
            r.animate(morphs={morph: w})
        got = r.read_vertices(0, len(v0))
        assert not np.array_equal(want[:, :6], v0[first:first + n, :6])
        same_finite_bits(got[first:first + n], want)
        assert same_bits(got[:first], v0[:first]) and same_bits(got[first + n:], v0[first + n:])
        r.remove_morph(morph)
        if attached:
            r.remove_skin(skin)
        r.update_vertices(v0[first:first + n], first=first)


def bent_and_morphed(instance, levels, size=(64, 48)):
    """the sheet under a skin that carries a morph, both named in one animate: (desc, the host's vertices, scene, renderer, skin, morph)"""
    desc = instanced_sheets(12, seed=21) if levels == "two_level" else sheet_scene()
    j, sw = sheet_influences(desc.vertices)
    targets, bones = sheet_targets(desc.vertices), bend(0.4, lift=0.05)
    a, ra = renderer(instance, desc, levels, size)
    skin = ra.add_skin(N_ROOM, j, sw, 2)
    morph = ra.add_morph(N_ROOM, targets, skin=skin)
    ra.animate(morphs={morph: WEIGHTS}, poses={skin: bones})
    v1 = host_posed(host_morphed(desc.vertices, N_ROOM, N_SHEET, targets, WEIGHTS), N_ROOM, j, sw, bones)
    return desc, v1, a, ra, skin, morph


@pytest.mark.parametrize("levels", ["flat", "two_level"])
def test_fused_scene_equals_a_fresh_scene(instance, levels):
    desc, v1, a, ra, _, _ = bent_and_morphed(instance, levels)
    same_finite_bits(ra.read_vertices(0, len(v1)), as_rows(v1))
    b, rb = renderer(instance, with_vertices(desc, v1), levels)
    assert_same_hits(a, b, 50_000)
    assert_same_render(ra, rb)


# ---- 4: a free-standing morph, a morphed skin and a plain skin in one call -----------------------------------------------------
FIRST_A, N_A = N_ROOM, 300                     # a free-standing morph
FIRST_B, N_B = N_ROOM + 400, 300               # a skin that carries a morph
FIRST_C = N_ROOM + 800                         # a plain skin, to the sheet's end
N_C = N_SHEET - 800


def three_parts(r, vertices):
    rng = np.random.default_rng(2)
    ta = [random_target(rng, N_A, None, 0.01), random_target(rng, N_A, 50, 0.02)]
    tb = [random_target(rng, N_B, 120, 0.02), random_target(rng, N_B, None, 0.01), random_target(rng, N_B, 0)]
    jb, wb = sheet_influences(vertices, FIRST_B, N_B)
    jc, wc = sheet_influences(vertices, FIRST_C, N_C)
    ma = r.add_morph(FIRST_A, ta)
    sb = r.add_skin(FIRST_B, jb, wb, 2)
    mb = r.add_morph(FIRST_B, tb, skin=sb)
    sc = r.add_skin(FIRST_C, jc, wc, 2)
    return (ma, ta), (sb, jb, wb, mb, tb), (sc, jc, wc)


def host_three(vertices, parts, wa, wb, bones_b, bones_c):
    (_, ta), (_, jb, sb, _, tb), (_, jc, sc) = parts
    v = host_morphed(vertices, FIRST_A, N_A, ta, wa)
    v = host_posed(host_morphed(v, FIRST_B, N_B, tb, wb), FIRST_B, jb, sb, bones_b)
    return host_posed(v, FIRST_C, jc, sc, bones_c)


def test_one_call_names_a_morph_a_morphed_skin_and_a_plain_skin(instance):
    desc = sheet_scene()
    a, ra = renderer(instance, desc)
    parts = three_parts(ra, desc.vertices)
    (ma, _), (sb, _, _, mb, _), (sc, _, _) = parts
    wa, wb = np.array([1.0, -0.5], np.float32), np.array([0.5, 1.5, 3.0], np.float32)
    bones_b, bones_c = np.stack([hinge(0.0, lift=0.05), hinge(0.1)]), bend(-0.3)
    ra.animate(morphs={mb: wb, ma: wa}, poses={sc: bones_c, sb: bones_b})
    v1 = host_three(desc.vertices, parts, wa, wb, bones_b, bones_c)
    got = ra.read_vertices(0, len(v1))
    same_finite_bits(got, as_rows(v1))
    for gap in (slice(0, FIRST_A), slice(FIRST_A + N_A, FIRST_B), slice(FIRST_B + N_B, FIRST_C)):
        assert same_bits(got[gap], as_rows(desc.vertices)[gap])
    for lo, n in ((FIRST_A, N_A), (FIRST_B, N_B), (FIRST_C, N_C)):
        assert not np.array_equal(got[lo:lo + n, :6], as_rows(desc.vertices)[lo:lo + n, :6])
    c, rc = renderer(instance, desc)
    rc.update_vertices(v1[N_ROOM:], first=N_ROOM)                                                 # ONE update over the joined span
    ua, uc = ra.geometry_update_info(), rc.geometry_update_info()
    assert (ua.mode, ua.meshes_touched) == (uc.mode, uc.meshes_touched) == (abi.GEOMETRY_REFIT, 1) and ua.update_ms >= 0
    assert ua.box_area == pytest.approx(uc.box_area, rel=1e-5) and ua.box_area_built == pytest.approx(uc.box_area_built, rel=1e-5)
    assert_same_structure(a, c)
    b, rb = renderer(instance, with_vertices(desc, v1))
    assert_same_hits(a, b, 50_000)
    assert_same_render(ra, rb)


# ---- 5: pose() knows nothing of morphs; the bases stay -------------------------------------------------------------------------
def test_pose_ignores_the_morph_and_a_second_animate_starts_from_the_base(instance):
    desc, v1, a, ra, skin, morph = bent_and_morphed(instance, "flat")
    j, sw = sheet_influences(desc.vertices)
    bones = bend(-0.3)
    ra.pose({skin: bones})                                                                        # from the unmorphed bind pose, exactly as before
    v2 = host_posed(desc.vertices, N_ROOM, j, sw, bones)
    assert same_bits(ra.read_vertices(0, len(v2)), as_rows(v2))
    ra.animate(poses={skin: bones})                                                               # a named skin whose morph is not named: the same
    assert same_bits(ra.read_vertices(0, len(v2)), as_rows(v2))
    targets, w = sheet_targets(desc.vertices), np.array([-0.3, 0.2, 0.0], np.float32)
    ra.animate(morphs={morph: w}, poses={skin: bones})                                            # from the base, not from the last result
    v3 = host_posed(host_morphed(desc.vertices, N_ROOM, N_SHEET, targets, w), N_ROOM, j, sw, bones)
    same_finite_bits(ra.read_vertices(0, len(v3)), as_rows(v3))
    b, rb = renderer(instance, with_vertices(desc, v3))
    assert_same_hits(a, b, 50_000)
    assert_same_render(ra, rb)


def test_a_second_animate_of_a_free_standing_morph_starts_from_its_base(instance):
    desc, _, a, ra, morph = morphed(instance, "flat", "refit")
    targets, w = sheet_targets(desc.vertices), np.array([0.1, 0.9, -1.0], np.float32)
    ra.animate(morphs={morph: w})
    v2 = host_morphed(desc.vertices, N_ROOM, N_SHEET, targets, w)
    same_finite_bits(ra.read_vertices(0, len(v2)), as_rows(v2))


# ---- 6: refused arguments -----------------------------------------------------------------------------------------------------
def animation(morphs, poses):
    """(abi.Animation, what it points into) of [(morph, weights or None, n_targets)] and [(skin, bones or None, n_bones)]; None = a null array"""
    ws = [None if m[1] is None else np.ascontiguousarray(m[1], np.float32) for m in morphs or []]
    marr = (abi.MorphWeights * max(1, len(ws)))(*[abi.MorphWeights(m[0], None if w is None else w.ctypes.data, m[2]) for m, w in zip(morphs or [], ws)])
    parr, keep = pose_array(poses) if poses else (None, None)
    a = abi.Animation(None if morphs is None else C.cast(marr, C.c_void_p), len(morphs or []), None if parr is None else C.cast(parr, C.c_void_p), len(poses or []))
    return a, (ws, marr, parr, keep)


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
    rng = np.random.default_rng(1)
    j, sw = sheet_influences(desc.vertices, N_ROOM, 300)
    skin = r.add_skin(N_ROOM, j, sw, 2)                                                           # a skin with a morph,
    attached = r.add_morph(N_ROOM, [random_target(rng, 300, 40)], skin=skin)
    j2, sw2 = sheet_influences(desc.vertices, N_ROOM + 300, 100)
    bare = r.add_skin(N_ROOM + 300, j2, sw2, 2)                                                   # a skin without,
    free = r.add_morph(N_ROOM + 500, [random_target(rng, 100, None), random_target(rng, 100, 10)])   # and a free-standing morph (binding changes no vertex)
    assert (attached, free) == (0, 1)
    before, v_before = structure(a), r.read_vertices(0, len(desc.vertices))
    assert same_bits(v_before, as_rows(desc.vertices))
    lib, n_all = abi.lib(), len(desc.vertices)
    d = np.full((100, 3), 0.01, np.float32)
    far = N_ROOM + 700                                                                            # clear of everything that is there

    def add(first, n, entries, skin_id=-1, n_targets=None):
        arr, keep = target_array(entries) if entries is not None else (None, None)
        m = abi.Morph(first, n, None if arr is None else C.cast(arr, C.c_void_p), len(entries) if n_targets is None else n_targets, skin_id)
        return lib.glz_renderer_add_morph(r._h, C.cast(C.byref(m), C.c_void_p))

    dense, sparse = (None, d, d, 100), ([0, 5, 99], d[:3], d[:3], 3)
    assert lib.glz_renderer_add_morph(r._h, None) == abi.E_ARG and add(far, 100, None, n_targets=1) == abi.E_ARG          # null pointers
    assert add(far, 0, [sparse]) == abi.E_ARG                                                    # none
    assert add(n_all - 99, 100, [dense]) == abi.E_ARG and add(0xFFFFFFFF, 2, [sparse]) == abi.E_ARG                      # past the end (and a sum that wraps)
    assert add(far, 100, [dense], n_targets=0) == abi.E_ARG and add(far, 100, [dense], n_targets=65537) == abi.E_ARG    # n_targets out of 1 .. 65536
    assert add(far, 100, [([0, 100], d[:2], d[:2], 2)]) == abi.E_ARG                             # an entry index >= n_vertices
    assert add(far, 100, [([5, 5], d[:2], d[:2], 2)]) == abi.E_ARG and add(far, 100, [([6, 5], d[:2], d[:2], 2)]) == abi.E_ARG   # not strictly ascending
    assert add(far, 99, [dense]) == abi.E_ARG and add(far, 101, [dense]) == abi.E_ARG            # a dense target whose n is not n_vertices
    assert add(far, 100, [([0, 5], None, d[:2], 2)]) == abi.E_ARG and add(far, 100, [([0, 5], d[:2], None, 2)]) == abi.E_ARG     # null deltas where n > 0
    assert add(N_ROOM + 599, 10, [([0], d[:1], d[:1], 1)]) == abi.E_ARG and add(N_ROOM + 450, 51, [([0], d[:1], d[:1], 1)]) == abi.E_ARG   # overlaps a morph, at either end
    assert add(N_ROOM + 399, 10, [([0], d[:1], d[:1], 1)]) == abi.E_ARG and add(0, N_ROOM + 1, [([0], d[:1], d[:1], 1)]) == abi.E_ARG      # overlaps a skin
    assert add(N_ROOM + 300, 100, [dense], skin_id=bare + 5) == abi.E_ARG and add(N_ROOM + 300, 100, [dense], skin_id=-2) == abi.E_ARG    # an unknown skin
    assert add(N_ROOM, 300, [([0], d[:1], d[:1], 1)], skin_id=skin) == abi.E_ARG                 # a skin that already has a morph
    assert add(N_ROOM + 300, 99, [([0], d[:1], d[:1], 1)], skin_id=bare) == abi.E_ARG and add(N_ROOM + 301, 99, [([0], d[:1], d[:1], 1)], skin_id=bare) == abi.E_ARG   # not the skin's range
    assert lib.glz_renderer_remove_morph(r._h, free + 1) == abi.E_ARG and lib.glz_renderer_remove_morph(r._h, -1) == abi.E_ARG
    assert lib.glz_renderer_remove_skin(r._h, skin) == abi.E_ARG                                  # a skin that still carries a morph
    s = abi.Skin(N_ROOM + 550, 100, j2.ctypes.data, sw2.ctypes.data, 2)
    assert lib.glz_renderer_add_skin(r._h, C.cast(C.byref(s), C.c_void_p)) == abi.E_ARG           # a skin over a free-standing morph
    assert add(far, 100, [dense, (None, None, None, 0)]) == free + 1                              # (and one that is fine: a target with n == 0 is allowed)
    nxt = free + 1

    two = bend(0.4)
    w1, w2 = np.array([0.5], np.float32), np.array([0.5, 0.25], np.float32)
    bad = [(None, None),                                                                          # nothing named
           ([(free + 7, w2, 2)], None),                                                           # an unknown morph
           ([(free, w2, 2), (nxt, w2, 2), (free, w2, 2)], None),                                  # a morph named twice
           ([(free, None, 2)], None),                                                             # null weights
           ([(free, w2, 1)], None), ([(free, w2, 3)], None),                                      # n_targets not the morph's
           ([(attached, w1, 1)], None), ([(attached, w1, 1)], [(bare, two, 2)]),                  # an attached morph without its skin's pose
           ([(free, w2, 2)], [(bare + 9, two, 2)]), ([(free, w2, 2)], [(bare, two, 3)]), ([(free, w2, 2)], [(bare, None, 2)]),   # the pose checks
           ([(free, w2, 2)], [(bare, two, 2), (bare, two, 2)]), (None, [(bare, two, 3)])]
    cam = moved_camera(desc.camera)
    out = np.zeros((48, 64, 4), np.float32)
    frames = [np.zeros((48, 64, 4), np.float32) for _ in range(3)]
    v_rows = as_rows(desc.vertices)

    def state(vertices=None, camera=cam):
        return abi.PreviousState(None if camera is None else C.cast(C.byref(camera), C.c_void_p), None, 0, None if vertices is None else vertices.ctypes.data, 0,
                                 0 if vertices is None else len(vertices))

    def animate(an, mode=abi.GEOMETRY_REFIT):
        return lib.glz_renderer_animate(r._h, None if an is None else C.cast(C.byref(an), C.c_void_p), mode)

    def motion(st, an, result=out):
        return lib.glz_renderer_read_motion_animated(r._h, None if st is None else C.cast(C.byref(st), C.c_void_p), None if an is None else C.cast(C.byref(an), C.c_void_p),
                                                     None if result is None else result.ctypes.data)

    def reproject(st, an, result=out):
        return lib.glz_renderer_reproject_animated(r._h, None if st is None else C.cast(C.byref(st), C.c_void_p), None if an is None else C.cast(C.byref(an), C.c_void_p),
                                                   frames[0].ctypes.data, frames[1].ctypes.data, frames[2].ctypes.data, None, None if result is None else result.ctypes.data)

    for morphs, poses in bad:
        an, keep = animation(morphs, poses)
        assert animate(an) == abi.E_ARG, (morphs, poses)
        assert motion(state(), an) == abi.E_ARG and reproject(state(), an) == abi.E_ARG, (morphs, poses)
    null_arrays = abi.Animation(None, 1, None, 0)                                                 # a count with a null array
    assert animate(null_arrays) == abi.E_ARG and animate(abi.Animation(None, 0, None, 1)) == abi.E_ARG
    good, keep_good = animation([(free, w2, 2), (attached, w1, 1)], [(skin, two, 2)])
    assert animate(None) == abi.E_ARG and animate(good, 2) == abi.E_ARG                           # a null animation; an unknown mode
    for call in (motion, reproject):
        assert call(state(), None) == abi.E_ARG
        assert call(state(vertices=v_rows), good) == abi.E_ARG                                    # an animated state brings no vertices
        assert call(None, good) == abi.E_ARG and call(state(camera=None), good) == abi.E_ARG and call(state(), good, None) == abi.E_ARG
    with pytest.raises(ValueError):
        r.add_morph(far + 150, [(np.array([0, 1]), d[:2], d[:3])], n_vertices=10)
    with pytest.raises(glaze_amd.GlazeError):
        r.animate(morphs={free: w1})

    assert_same_bytes(before, structure(a))
    assert same_bits(r.read_vertices(0, n_all), v_before)
    assert add(far + 150, 10, [([0], d[:1], d[:1], 1)]) == nxt + 1                                # no refused call took an id
    for x in (r, ref):
        x.step(4)
    assert np.array_equal(bits(r.read_hdr()), bits(ref.read_hdr()))                              # the accumulation went on, on the same scene
    assert np.array_equal(bits(r.read_result()), bits(ref.read_result()))


# ---- 7: the other devices of set_devices --------------------------------------------------------------------------------------
@pytest.mark.parametrize("levels", ["flat", "two_level"])
@pytest.mark.parametrize("devices_first", [True, False])
def test_loopback_devices_follow_animate(instance, loopback, levels, devices_first):
    desc = instanced_sheets(10, seed=9)
    r = glaze_amd.RayTraceRenderer.new(instance, make_scene(instance, desc, levels), 136, 200)
    if devices_first:
        r.set_devices([instance.device] * 2)
    parts = three_parts(r, desc.vertices)
    (ma, _), (sb, _, _, mb, _), (sc, _, _) = parts
    wa, wb = np.array([1.0, -0.5], np.float32), np.array([0.5, 1.5, 3.0], np.float32)
    bones_b, bones_c = np.stack([hinge(0.0, lift=0.05), hinge(0.1)]), bend(-0.3)
    r.animate(morphs={ma: -wa, mb: wb[::-1].copy()}, poses={sb: bones_c, sc: bones_b})
    if not devices_first:
        r.set_devices([instance.device] * 2)                                                     # the replica is made of the animated scene, morphs included
    r.animate(morphs={ma: wa, mb: wb}, poses={sb: bones_b, sc: bones_c})
    v1 = host_three(desc.vertices, parts, wa, wb, bones_b, bones_c)
    one = glaze_amd.RayTraceRenderer.new(instance, make_scene(instance, with_vertices(desc, v1), levels), 136, 200)
    assert_same_render(r, one)
    assert np.array_equal(r.read_rgba8(), one.read_rgba8())


# ---- 8: motion and reprojection that follow an animation ----------------------------------------------------------------------
@pytest.mark.parametrize("levels", ["flat", "two_level"])
@pytest.mark.parametrize("with_transforms", [False, True])
def test_animated_motion_and_reprojection_equal_the_host_made_ones(instance, levels, with_transforms):
    desc = instanced_sheets(10, seed=31) if levels == "two_level" else sheet_scene()
    desc.camera = make_camera(position=(0, 0.35, -0.35), target=(0, -0.4, 0.55), fovx=FOVX, near=1e-3, far=100.0)
    _, r = renderer(instance, desc, levels)
    parts = three_parts(r, desc.vertices)
    (ma, ta), (sb, jb, swb, mb, tb), (sc, jc, swc) = parts
    wa, wb = np.array([1.0, -0.5], np.float32), np.array([0.5, 1.5, 3.0], np.float32)
    r.animate(morphs={ma: wa, mb: wb}, poses={sb: np.stack([hinge(0.0, lift=0.05), hinge(0.3)]), sc: bend(0.4)})
    pa, pb = np.array([0.2, 0.4], np.float32), np.array([-0.5, 0.5, 0.0], np.float32)             # the previous frame's
    prev_b, prev_c = np.stack([hinge(0.0), hinge(0.1)]), bend(0.1, lift=0.05)
    cam = moved_camera(desc.camera, shift=(0.1, 0.05, -0.1), turn=(0.1, -0.05, 0.1))
    t0 = moved_transforms(desc.transforms, 5) if with_transforms else None
    # the previous vertices over the span, on the host: the current ones (the gaps keep them), then each part as the previous animation makes it
    bind = desc.vertices
    span = as_vertices(r.read_vertices(FIRST_A, N_SHEET))
    span[:N_A] = as_vertices(glaze_amd.host_morph(bind[FIRST_A:FIRST_A + N_A], ta, pa))
    lo = FIRST_B - FIRST_A
    span[lo:lo + N_B] = as_vertices(glaze_amd.host_skin(glaze_amd.host_morph(bind[FIRST_B:FIRST_B + N_B], tb, pb), jb, swb, prev_b))
    span[FIRST_C - FIRST_A:] = as_vertices(glaze_amd.host_skin(bind[FIRST_C:FIRST_C + N_C], jc, swc, prev_c))
    want = r.read_motion(cam, t0, prev_vertices=span, first_vertex=FIRST_A)
    got = r.read_motion(cam, t0, prev_morphs={ma: pa, mb: pb}, prev_poses={sb: prev_b, sc: prev_c})
    assert np.array_equal(bits(got), bits(want))
    if levels == "flat":                                                                         # (the camera looks at the sheet there)
        assert not np.array_equal(bits(got), bits(r.read_motion(cam, t0)))                       # the animation did move what it sees
    one = r.read_motion(cam, t0, prev_morphs={ma: pa})                                           # one free-standing morph: its own span
    span_a = as_vertices(glaze_amd.host_morph(bind[FIRST_A:FIRST_A + N_A], ta, pa))
    assert np.array_equal(bits(one), bits(r.read_motion(cam, t0, prev_vertices=span_a, first_vertex=FIRST_A)))
    rng = np.random.default_rng(3)
    color = rng.random((48, 64, 4)).astype(np.float32)
    aov0, aov1 = r.read_aov(0), r.read_aov(1)
    for params in ({}, dict(depth_tolerance=0.5)):
        got = r.reproject(cam, color, aov0, aov1, t0, prev_morphs={ma: pa, mb: pb}, prev_poses={sb: prev_b, sc: prev_c}, **params)
        want = r.reproject(cam, color, aov0, aov1, t0, prev_vertices=span, first_vertex=FIRST_A, **params)
        assert np.array_equal(bits(got), bits(want))
        if levels == "flat" and not with_transforms and params:
            assert (got[..., 3] > 0).any()                                                       # (and it is no empty frame that agrees)


# ---- 9: whoever holds the scene sees morphs -----------------------------------------------------------------------------------
def test_the_scene_handle_sees_morphs(instance):
    """as the skin test of that name: the second holder is the scene handle, which outlives the renderer"""
    desc, v1, a, ra, _ = morphed(instance, "flat", "refit")
    b = make_scene(instance, with_vertices(desc, v1))
    assert_same_hits(a, b, 20_000)
    del ra                                                                                        # the scene, its morph and its vertices stay
    assert_same_hits(a, b, 20_000, seed=1)
