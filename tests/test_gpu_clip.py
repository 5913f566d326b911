"""Skeletons and clips under a live renderer (glz_renderer_add_skeleton, glz_renderer_add_clip, glz_renderer_play, glz_debug_clip_bones).

k_clip_bones must leave, bit for bit, the bone table the host makes of glz_host_clip_bones (tests/test_clip_host.py holds that reference
to the specification) -- pack_bone's rows for a linear skin, glz_host_bone_dual_quats' for a skin in dual-quaternion mode -- and a
played scene must be the scene glz_renderer_pose_skins / glz_renderer_animate leave when they are given those bones and weights: vertex
for vertex, hit for hit and pixel for pixel.

The skeletons are the smallest at which the kernel can go wrong: one bone (one level, one lane); a chain of 70 (more levels than a
wave has lanes, one bone a level, a barrier between every pair); 300 bones in two levels (a level wider than the block: the stride
loop runs twice); a tree of 7 with two roots."""
import ctypes as C

import numpy as np
import pytest

import glaze_amd
from glaze_amd import abi

import clip_cases as cc
from test_gpu_morph import sheet_targets
from test_gpu_normals import host_normals
from test_gpu_skin import N_SHEET, as_rows, as_vertices, loopback, renderer, same_finite_bits  # noqa: F401
from test_gpu_vertex_update import N_ROOM, assert_same_bytes, assert_same_hits, assert_same_render, instanced_sheets, make_scene, sheet_scene, structure, with_vertices

pytestmark = pytest.mark.gpu

F = np.float32
SIZE = (32, 24)
SHAPES = {"one": lambda rng: cc.chain(1), "chain70": lambda rng: cc.chain(70), "star300": lambda rng: cc.star(300), "tree7": lambda rng: cc.random_tree(rng, 7, roots=2)}
BLENDS = ["linear", "dual_quaternion"]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


class Character:
    """A skin over the scene's vertices [first, first + n) with a skeleton of `shape` and one clip on it; gentle: bones that stay near
    the identity (the scene stays a scene: what the hit and render tests need)"""

    def __init__(self, r, vertices, shape, first=N_ROOM, n=300, seed=0, blend="linear", n_keys=2, morph=False, gentle=False, scaled=True):
        rng = np.random.default_rng(seed)
        self.r, self.first, self.n, self.blend = r, first, n, blend
        self.parents = SHAPES[shape](rng)
        k = self.n_bones = len(self.parents)
        self.joints = rng.integers(0, k, (n, 4)).astype(np.uint16)
        self.joints[0] = (0, k - 1, k - 1, 0)                                                    # bone 0 and the last one
        w = rng.uniform(0.1, 1.0, (n, 4))
        self.weights = (w / w.sum(1, keepdims=True)).astype(F)
        self.bind = as_rows(vertices)[first:first + n].copy()
        self.skin = r.add_skin(first, self.joints, self.weights, k, blend)
        self.targets = sheet_targets(vertices, first, n) if morph else None
        self.morph = r.add_morph(first, self.targets, skin=self.skin) if morph else None
        if gentle:
            self.inverse_bind, self.root = np.tile(np.eye(4, dtype=F).reshape(16), (k, 1)), None
            clip = cc.random_clip(rng, k, n_keys, scaled, 3 if morph else 0, reach=0.02, turn=0.03)
        else:
            self.inverse_bind, self.root = cc.random_rigid(rng, k, reach=0.2), cc.random_rigid(rng, 1, reach=0.2)[0]
            clip = cc.random_clip(rng, k, n_keys, scaled, 3 if morph else 0, reach=0.05, turn=0.3)
        self.times, self.tr, self.ro, self.sc, self.mw = clip
        self.skeleton = r.add_skeleton(self.skin, self.parents, self.inverse_bind, self.root)
        self.clip = r.add_clip(self.skeleton, self.times, self.tr, self.ro, self.sc, self.mw)
        self._host = {}

    def host(self, t):
        """(bones, weights or None) of glz_host_clip_bones at t: computed once a time"""
        key = F(t).tobytes()
        if key not in self._host:
            got = glaze_amd.host_clip_bones(self.parents, self.inverse_bind, self.times, self.tr, self.ro, t, self.sc, self.mw, self.root)
            self._host[key] = got if self.mw is not None else (got, None)
        return self._host[key]

    def host_vertices(self, t, blend=None):
        """the skin's vertices as the host references make them of the clip at t"""
        bones, weights = self.host(t)
        base = self.bind if weights is None else glaze_amd.host_morph(self.bind, self.targets, weights)
        return glaze_amd.host_skin(base, self.joints, self.weights, bones, blend or self.blend)

    def read(self):
        return self.r.read_vertices(self.first, self.n)


@pytest.fixture
def sheet(instance):
    desc = sheet_scene()
    scene, r = renderer(instance, desc, size=SIZE)
    return desc, scene, r


# ---- 1: the kernel's tables against the host reference --------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(SHAPES))
def test_bone_table_equals_the_packed_host_bones(sheet, shape):
    desc, _, r = sheet
    c = Character(r, desc.vertices, shape, seed=1)
    before = r.read_vertices(0, len(desc.vertices))
    for t in cc.times_around(c.times):
        got = r.debug_clip_bones(c.clip, t, c.n_bones)
        want = cc.pack_rows(c.host(t)[0])
        assert np.isfinite(want).all() and same_bits(got, want), (shape, float(t))
    assert same_bits(r.read_vertices(0, len(desc.vertices)), before)                             # the hook writes no vertex


@pytest.mark.parametrize("shape", list(SHAPES))
def test_bone_table_equals_the_host_dual_quaternions(sheet, shape):
    desc, _, r = sheet
    c = Character(r, desc.vertices, shape, seed=2, blend="dual_quaternion")
    for t in cc.times_around(c.times):
        got = r.debug_clip_bones(c.clip, t, c.n_bones, blend="dual_quaternion")
        want = glaze_amd.host_bone_dual_quats(c.host(t)[0])
        assert np.isfinite(want).all() and same_bits(got, want), (shape, float(t))


# ---- 2: play against the host references and against pose -----------------------------------------------------------------------
@pytest.mark.parametrize("blend", BLENDS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_play_equals_the_host_skin_and_pose_of_the_host_bones(sheet, shape, blend):
    desc, _, r = sheet
    v0 = as_rows(desc.vertices)
    c = Character(r, desc.vertices, shape, first=N_ROOM + 5, n=257, seed=3, blend=blend, scaled=blend == "linear")
    for t in cc.times_around(c.times):
        r.play([(c.clip, t)])
        played = r.read_vertices(0, len(v0))
        want = v0.copy()
        want[c.first:c.first + c.n] = c.host_vertices(t)
        assert not np.array_equal(want[c.first:c.first + c.n, :6], v0[c.first:c.first + c.n, :6])
        same_finite_bits(played, want)                                                           # and outside the range: untouched
        assert np.isfinite(played).all()
        r.pose({c.skin: c.host(t)[0]})
        assert same_bits(r.read_vertices(0, len(v0)), played), (shape, blend, float(t))


@pytest.mark.parametrize("blend", BLENDS)
def test_a_weight_track_equals_animate_with_the_lerped_weights(sheet, blend):
    desc, _, r = sheet
    c = Character(r, desc.vertices, "tree7", n=N_SHEET, seed=4, blend=blend, n_keys=3, morph=True, gentle=True)
    for t in cc.times_around(c.times):
        bones, weights = c.host(t)
        table, wtable = r.debug_clip_bones(c.clip, t, c.n_bones, blend=blend, n_targets=3)
        assert same_bits(wtable, weights)
        assert same_bits(table, cc.pack_rows(bones) if blend == "linear" else glaze_amd.host_bone_dual_quats(bones))
        r.play([(c.clip, t)])
        played = c.read()
        same_finite_bits(played, c.host_vertices(t))
        r.animate(morphs={c.morph: weights}, poses={c.skin: bones})
        assert same_bits(c.read(), played), (blend, float(t))
    assert not same_bits(played, glaze_amd.host_skin(c.bind, c.joints, c.weights, c.host(t)[0], blend))   # the morph did take part


# ---- 3: a crowd in one call -----------------------------------------------------------------------------------------------------
def test_three_skins_in_one_call_leave_the_gaps_alone(sheet):
    desc, _, r = sheet
    v0 = as_rows(desc.vertices)
    crowd = [Character(r, desc.vertices, "one", first=N_ROOM + 3, n=100, seed=5), Character(r, desc.vertices, "chain70", first=N_ROOM + 200, n=257, seed=6),
             Character(r, desc.vertices, "star300", first=N_ROOM + 600, n=300, seed=7, blend="dual_quaternion", scaled=False)]
    times = [c.times[0] + F(f) * (c.times[1] - c.times[0]) for c, f in zip(crowd, (0.25, 0.5, 1.5))]
    alone = []
    for c, t in zip(crowd, times):
        r.play([(c.clip, t)])
        alone.append(c.read())
        same_finite_bits(alone[-1], c.host_vertices(t))
    r.update_vertices(v0[N_ROOM:], first=N_ROOM)                                                  # the sheet as it was
    r.play([(c.clip, t) for c, t in reversed(list(zip(crowd, times)))])
    got = r.read_vertices(0, len(v0))
    want = v0.copy()
    for c, a in zip(crowd, alone):
        want[c.first:c.first + c.n] = a
    assert same_bits(got, want)                                                                   # each its own single play; gaps and room untouched
    u = r.geometry_update_info()                                                                  # ONE update of the structure
    assert (u.mode, u.meshes_touched) == (abi.GEOMETRY_REFIT, 1) and u.update_ms >= 0 and u.box_area > 0
    assert r.debug_clip_timing([(c.clip, t) for c, t in zip(crowd, times)], reps=2) > 0
    assert same_bits(r.read_vertices(0, len(v0)), got)                                            # the timing hook writes no vertex


# ---- 4: nothing is kept between calls -------------------------------------------------------------------------------------------
def test_set_skin_blend_between_two_plays_switches_the_table_layout(sheet):
    desc, _, r = sheet
    c = Character(r, desc.vertices, "tree7", seed=8, scaled=False)
    t = c.times[0] + F(0.5) * (c.times[1] - c.times[0])
    r.play([(c.clip, t)])
    same_finite_bits(c.read(), c.host_vertices(t, "linear"))
    r.set_skin_blend(c.skin, "dual_quaternion")
    assert same_bits(r.debug_clip_bones(c.clip, t, c.n_bones, blend="dual_quaternion"), glaze_amd.host_bone_dual_quats(c.host(t)[0]))
    r.play([(c.clip, t)])
    same_finite_bits(c.read(), c.host_vertices(t, "dual_quaternion"))
    assert not same_bits(c.host_vertices(t, "linear"), c.host_vertices(t, "dual_quaternion"))
    r.set_skin_blend(c.skin, "linear")
    assert same_bits(r.debug_clip_bones(c.clip, t, c.n_bones), cc.pack_rows(c.host(t)[0]))
    r.play([(c.clip, t)])
    same_finite_bits(c.read(), c.host_vertices(t, "linear"))


def test_a_second_play_starts_from_the_bind_pose(sheet):
    desc, _, r = sheet
    c = Character(r, desc.vertices, "chain70", seed=9)
    r.play([(c.clip, c.times[0])])
    r.update_vertices(c.read() * F(1.5), first=c.first)                                          # over the skinned range: allowed
    r.play([(c.clip, c.times[1])])
    same_finite_bits(c.read(), c.host_vertices(c.times[1]))
    clip2 = r.add_clip(c.skeleton, c.times[:1], c.tr[:1], c.ro[:1], c.sc[:1])                    # a second clip on the same skeleton: key 0 alone
    r.play([(clip2, 0.0)])
    same_finite_bits(c.read(), c.host_vertices(c.times[0]))
    r.remove_clip(clip2)
    with pytest.raises(glaze_amd.GlazeError):
        r.play([(clip2, 0.0)])


# ---- 5: a played scene is the scene created with the host-made vertices ---------------------------------------------------------
@pytest.mark.parametrize("levels,mode", [("flat", "refit"), ("flat", "rebuild"), ("two_level", "refit"), ("two_level", "rebuild")])
def test_played_scene_equals_a_fresh_scene(instance, levels, mode):
    desc = instanced_sheets(6, seed=21) if levels == "two_level" else sheet_scene()
    a, ra = renderer(instance, desc, levels, SIZE)
    c = Character(ra, desc.vertices, "tree7", n=N_SHEET, seed=10, gentle=True)
    t = c.times[0] + F(0.37) * (c.times[1] - c.times[0])
    ra.play([(c.clip, t)], mode)
    v1 = desc.vertices.copy()
    v1[c.first:c.first + c.n] = as_vertices(c.host_vertices(t))
    assert not np.array_equal(as_rows(v1)[N_ROOM:, :6], as_rows(desc.vertices)[N_ROOM:, :6])
    u = ra.geometry_update_info()
    assert u.mode == (abi.GEOMETRY_REFIT if mode == "refit" else abi.GEOMETRY_REBUILD) and u.update_ms >= 0
    b, rb = renderer(instance, with_vertices(desc, v1), levels, SIZE)
    assert_same_hits(a, b, 20_000)
    assert_same_render(ra, rb)


def test_a_normal_set_over_the_range_runs_after_play(sheet):
    desc, a, r = sheet
    c = Character(r, desc.vertices, "tree7", n=N_SHEET, seed=11, gentle=True)
    r.add_normals(N_ROOM, N_SHEET)
    t = c.times[1] + F(1)
    r.play([(c.clip, t)])
    v1 = desc.vertices.copy()
    v1[c.first:c.first + c.n] = as_vertices(c.host_vertices(t))
    want = host_normals(desc, v1, N_ROOM, N_SHEET)
    assert same_bits(r.read_vertices(0, len(want)), as_rows(want))
    assert not same_bits(as_rows(want)[N_ROOM:, 3:6], as_rows(v1)[N_ROOM:, 3:6])


# ---- 6: the other devices of set_devices ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("devices_first", [True, False])
def test_loopback_devices_follow_a_play(instance, loopback, devices_first):
    desc = instanced_sheets(6, seed=9)
    r = glaze_amd.RayTraceRenderer.new(instance, make_scene(instance, desc, "flat"), 32, 32)
    if devices_first:
        r.set_devices([instance.device] * 2)
    c = Character(r, desc.vertices, "tree7", n=N_SHEET, seed=12, gentle=True, morph=True)
    r.play([(c.clip, c.times[0])])
    if not devices_first:
        r.set_devices([instance.device] * 2)                                                     # the replica is made with the skeleton and the clip, under the same ids
    t = c.times[0] + F(0.6) * (c.times[1] - c.times[0])
    r.play([(c.clip, t)])
    v1 = desc.vertices.copy()
    v1[c.first:c.first + c.n] = as_vertices(c.host_vertices(t))
    one = glaze_amd.RayTraceRenderer.new(instance, make_scene(instance, with_vertices(desc, v1), "flat"), 32, 32)
    assert_same_render(r, one)
    assert np.array_equal(r.read_rgba8(), one.read_rgba8())
    clip2 = r.add_clip(c.skeleton, c.times, c.tr, c.ro)                                          # ids count on alike on every device
    assert clip2 == c.clip + 1
    r.remove_skeleton(c.skeleton)                                                                 # and go alike: the skin is free again everywhere
    r.remove_morph(c.morph)
    r.remove_skin(c.skin)


# ---- 7: refused arguments -------------------------------------------------------------------------------------------------------
def test_refused_arguments_change_nothing(sheet):
    desc, a, r = sheet
    c = Character(r, desc.vertices, "tree7", n=N_SHEET, seed=13, gentle=True, morph=True)
    r.play([(c.clip, c.times[0])])
    before, v_before, u_before = structure(a), r.read_vertices(0, len(desc.vertices)), r.geometry_update_info()
    lib = abi.lib()
    clip2 = r.add_clip(c.skeleton, c.times, c.tr, c.ro)                                          # a second clip of the same skeleton

    def play(entries, n=None, mode=abi.GEOMETRY_REFIT):
        arr = None if entries is None else (abi.Play * max(1, len(entries)))(*[abi.Play(k, t) for k, t in entries])
        return lib.glz_renderer_play(r._h, None if arr is None else C.cast(arr, C.c_void_p), len(entries or [0]) if n is None else n, mode)

    assert play(None) == abi.E_ARG and play([(c.clip, 0.0)], n=0) == abi.E_ARG                  # a null pointer, none named
    assert play([(clip2 + 1, 0.0)]) == abi.E_ARG and play([(-1, 0.0)]) == abi.E_ARG              # an unknown clip
    assert play([(c.clip, 0.0), (clip2, 0.5)]) == abi.E_ARG                                      # two clips of one skeleton
    assert play([(c.clip, float("nan"))]) == abi.E_ARG and play([(c.clip, float("inf"))]) == abi.E_ARG
    assert play([(c.clip, 0.0)], mode=2) == abi.E_ARG                                            # an unknown mode
    with pytest.raises(glaze_amd.GlazeError):                                                    # a weight track with another target count
        r.add_clip(c.skeleton, c.times, c.tr, c.ro, morph_weights=np.zeros((len(c.times), 4), F))
    with pytest.raises(glaze_amd.GlazeError):                                                    # a second skeleton on a skin
        r.add_skeleton(c.skin, c.parents, c.inverse_bind)
    with pytest.raises(glaze_amd.GlazeError):                                                    # remove_skin under a skeleton
        r.remove_skin(c.skin)
    with pytest.raises(glaze_amd.GlazeError):                                                    # remove_morph under a clip's weight track
        r.remove_morph(c.morph)
    j = np.zeros((N_ROOM, 4), np.uint16)
    bare = r.add_skin(0, j, np.full((N_ROOM, 4), 0.25, F), 3)                                    # a skin of 3 bones: the room
    with pytest.raises(glaze_amd.GlazeError):                                                    # n_bones not the skin's
        r.add_skeleton(bare, c.parents, c.inverse_bind)
    with pytest.raises(glaze_amd.GlazeError):                                                    # a parent that does not come before its bone
        r.add_skeleton(bare, [-1, 2, 0], c.inverse_bind[:3])
    sk = r.add_skeleton(bare, [-1, 0, 0], c.inverse_bind[:3])
    with pytest.raises(glaze_amd.GlazeError):                                                    # a weight track on a skin without a morph
        r.add_clip(sk, c.times, c.tr[:, :3], c.ro[:, :3], morph_weights=c.mw)
    with pytest.raises(glaze_amd.GlazeError):                                                    # times that do not ascend
        r.add_clip(sk, c.times[::-1], c.tr[:, :3], c.ro[:, :3])
    with pytest.raises(glaze_amd.GlazeError):
        r.remove_clip(clip2 + 1)
    with pytest.raises(glaze_amd.GlazeError):
        r.remove_skeleton(sk + 1)
    assert lib.glz_renderer_add_skeleton(r._h, None) == abi.E_ARG and lib.glz_renderer_add_clip(r._h, None) == abi.E_ARG
    assert r.add_clip(sk, c.times, c.tr[:, :3], c.ro[:, :3]) == clip2 + 1                        # ids count up; refusals took none
    assert_same_bytes(before, structure(a))
    assert same_bits(r.read_vertices(0, len(desc.vertices)), v_before)
    u = r.geometry_update_info()                                                                  # still the play's
    assert (u.mode, u.meshes_touched, u.update_ms) == (u_before.mode, u_before.meshes_touched, u_before.update_ms)
    assert u.box_area == pytest.approx(u_before.box_area, rel=1e-5) and u.box_area_built == pytest.approx(u_before.box_area_built, rel=1e-5)


# ---- 8: pose and animate on a skin that has a skeleton ---------------------------------------------------------------------------
def test_pose_and_animate_work_as_before_on_a_skin_with_a_skeleton(sheet):
    desc, _, r = sheet
    c = Character(r, desc.vertices, "tree7", n=N_SHEET, seed=14, gentle=True, morph=True)
    r.play([(c.clip, c.times[1])])
    rng = np.random.default_rng(15)
    bones = cc.random_rigid(rng, c.n_bones, reach=0.05)
    r.pose({c.skin: bones})
    same_finite_bits(c.read(), glaze_amd.host_skin(c.bind, c.joints, c.weights, bones))
    weights = np.array([0.5, -0.25, 1.0], F)
    r.animate(morphs={c.morph: weights}, poses={c.skin: bones})
    same_finite_bits(c.read(), glaze_amd.host_skin(glaze_amd.host_morph(c.bind, c.targets, weights), c.joints, c.weights, bones))
