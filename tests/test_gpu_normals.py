"""Vertex normals recomputed on the device (glz_renderer_add_normals, glz_renderer_remove_normals).

Two rules, as in test_gpu_skin.py.  k_face_vectors and k_vertex_normals must give, bit for bit, the normals glz_host_vertex_normals gives
(tests/test_normals_host.py holds that reference to the specification).  And a scene whose normals the device made -- after a pose, an
animate or new positions from the caller -- must be, hit for hit and pixel for pixel, the scene created fresh with the vertices the host
references give: host_skin / host_morph, then host_vertex_normals."""
import ctypes as C

import numpy as np
import pytest

import glaze_amd
from glaze_amd import abi
from glaze_amd.scene_desc import INSTANCE_DTYPE, MESH_DTYPE, VERTEX_DTYPE, make_light, make_material
from glaze_amd.scenes import cube_scene
from oracle.pyoracle import OracleRenderer, OracleScene

from test_gpu_morph import WEIGHTS, host_morphed, sheet_targets
from test_gpu_skin import N_SHEET, as_rows, as_vertices, bend, host_posed, loopback, renderer, same_finite_bits, sheet_influences  # noqa: F401
from test_gpu_vertex_update import (N_ROOM, assert_same_bytes, assert_same_hits, assert_same_render, assert_same_structure, bits, instanced_sheets, make_scene,
                                    render, sheet, sheet_scene, structure, waved, with_vertices)

pytestmark = pytest.mark.gpu


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def host_normals(desc, vertices, first, n, groups=None):
    """the whole vertex array with the normals of [first, first + n) as glz_host_vertex_normals makes them of `vertices`' positions"""
    v = np.ascontiguousarray(vertices, VERTEX_DTYPE).copy()
    v[first:first + n] = as_vertices(glaze_amd.host_vertex_normals(v, desc.indices, desc.meshes, first, n, groups))
    return v


# ---- 1: the kernels against the host reference -----------------------------------------------------------------------------------
def room_with(v, idx):
    """sheet_scene's room with another mesh in the sheet's place"""
    d = cube_scene(material_type=abi.MAT_UBER)
    d.materials.append(make_material("mesh", mtype=abi.MAT_UBER, diffuse_mul=(230, 200, 170), diffuse=1))
    d.vertices = np.concatenate([d.vertices, v])
    d.indices = np.concatenate([d.indices, np.asarray(idx, np.uint32) + np.uint32(N_ROOM)])
    d.meshes = np.array([(0, 2, 0, 36), (1, 3, 36, len(idx))], MESH_DTYPE)
    d.instances = np.array([(0, 0), (1, 0)], INSTANCE_DTYPE)
    d.lights.append(make_light(abi.LIGHT_SUN, "sun", direction=(0.2, -0.7, 0.4), intensity=0.5))
    return d


def torus(n=16, centre=(0.0, -0.3, 0.55), big=0.25, small=0.08):
    """a closed n x n grid: every vertex in six triangles, so every slice's rows are as long as the slice is wide"""
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    a, b = 2 * np.pi * i / n, 2 * np.pi * j / n
    v = np.zeros(n * n, VERTEX_DTYPE)
    ring = big + small * np.cos(b)
    v["vv"] = (np.stack([ring * np.cos(a), small * np.sin(b), ring * np.sin(a)], -1) + np.array(centre)).reshape(-1, 3).astype(np.float32)
    v["vn"] = (0.0, 1.0, 0.0)
    v["vt"] = np.stack([i / n, j / n], -1).reshape(-1, 2)
    idx = np.arange(n * n, dtype=np.uint32).reshape(n, n)
    p, q, r, s = idx, np.roll(idx, -1, 1), np.roll(np.roll(idx, -1, 0), -1, 1), np.roll(idx, -1, 0)
    return v, np.stack([p, q, r, p, r, s], -1).reshape(-1)


def fan(k=200, pole=(0.0, -0.2, 0.55), radius=0.3, y=-0.4):
    """k triangles around one pole: one row of k among rows of 2"""
    ang = 2 * np.pi * np.arange(k) / k
    v = np.zeros(k + 1, VERTEX_DTYPE)
    v["vv"][0] = pole
    v["vv"][1:] = np.stack([pole[0] + radius * np.cos(ang), np.full(k, y), pole[2] + radius * np.sin(ang)], -1).astype(np.float32)
    v["vn"] = (0.0, 1.0, 0.0)
    v["vt"][1:] = np.stack([ang / (2 * np.pi), np.ones(k)], -1)
    ring = 1 + np.arange(k, dtype=np.uint32)
    return v, np.stack([np.zeros(k, np.uint32), np.roll(ring, -1), ring], -1).reshape(-1)


def waved_positions(desc):
    """the sheet waved, under the flat sheet's normals: what the rule has to replace"""
    v = waved(desc.vertices)
    v["vn"][N_ROOM:] = desc.vertices["vn"][N_ROOM:]
    return with_vertices(desc, v)


SHAPES = {
    "sheet": lambda: (waved_positions(sheet_scene()), N_SHEET, None),                     # 17 full slices and one lane, rows of 1 .. 6
    "half": lambda: (waved_positions(sheet_scene()), 545, None),                          # faces with corners outside the range
    "torus": lambda: (room_with(*torus()), 256, None),                                    # four full slices, every row 6: the unmasked path
    "fan": lambda: (room_with(*fan()), 201, None),                                        # the masked path with a long loop
    "groups": lambda: (waved_positions(sheet_scene()), N_SHEET, np.random.default_rng(11).integers(0, N_SHEET - 5, N_SHEET).astype(np.uint32)),
}


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("offset", [0, 5])
def test_kernels_equal_the_host_reference(instance, shape, offset):
    desc, n, groups = SHAPES[shape]()
    first, n = N_ROOM + offset, n - offset
    if groups is not None:
        groups = groups[:n]
    v0 = as_rows(desc.vertices)
    _, r = renderer(instance, desc)
    r.add_normals(first, n, groups)
    got = r.read_vertices(0, len(v0))
    want = as_rows(host_normals(desc, desc.vertices, first, n, groups))
    assert not same_bits(want[first:first + n, 3:6], v0[first:first + n, 3:6])
    same_finite_bits(got[first:first + n], want[first:first + n])
    assert same_bits(got[:, 0:3], v0[:, 0:3]) and same_bits(got[:, 6:8], v0[:, 6:8])              # position and uv words: untouched
    assert same_bits(got[:first], v0[:first]) and same_bits(got[first + n:], v0[first + n:])      # and every vertex outside the set
    if shape == "torus" and offset == 0:
        assert np.isfinite(got).all() and np.allclose(np.linalg.norm(got[first:, 3:6], axis=1), 1.0, atol=1e-6)


# ---- 2: a scene with a set is the scene created with the host references' vertices -----------------------------------------------
def base_scene(levels):
    return instanced_sheets(12, seed=21) if levels == "two_level" else sheet_scene()


def posed_case(r, desc, mode):
    j, w = sheet_influences(desc.vertices)
    bones = bend(0.5, lift=0.05)
    skin = r.add_skin(N_ROOM, j, w, 2)
    r.add_normals(N_ROOM, N_SHEET)
    r.pose({skin: bones}, mode)
    return host_posed(desc.vertices, N_ROOM, j, w, bones)


def animated_case(r, desc, mode):
    j, w = sheet_influences(desc.vertices)
    targets, bones = sheet_targets(desc.vertices), bend(0.4, lift=0.05)
    r.add_normals(N_ROOM, N_SHEET)                                                                 # (before the skin: its bind pose has the rule's normals)
    bind = as_vertices(r.read_vertices(0, len(desc.vertices)))
    skin = r.add_skin(N_ROOM, j, w, 2)
    morph = r.add_morph(N_ROOM, targets, skin=skin)
    r.animate(morphs={morph: WEIGHTS}, poses={skin: bones}, mode=mode)
    return host_posed(host_morphed(bind, N_ROOM, N_SHEET, targets, WEIGHTS), N_ROOM, j, w, bones)


def updated_case(r, desc, mode):
    r.add_normals(N_ROOM, N_SHEET)
    v1 = waved(desc.vertices, 0.2, 0.4)
    v1["vn"][N_ROOM:] = np.random.default_rng(4).normal(size=(N_SHEET, 3)).astype(np.float32)     # garbage: the caller has positions only
    r.update_vertices(v1[N_ROOM:], first=N_ROOM, mode=mode)
    return v1


CASES = {"pose": posed_case, "animate": animated_case, "update_vertices": updated_case}


def run_case(instance, case, levels, mode, size=(64, 48)):
    """(desc, the host references' vertices, scene, renderer) after the case's calls"""
    desc = base_scene(levels)
    a, ra = renderer(instance, desc, levels, size)
    moved = CASES[case](ra, desc, mode)
    v1 = host_normals(desc, moved, N_ROOM, N_SHEET)
    assert not same_bits(as_rows(v1)[N_ROOM:, 3:6], as_rows(moved)[N_ROOM:, 3:6])                  # the rule's normals are not the ones the call wrote
    return desc, v1, a, ra


@pytest.mark.parametrize("levels,mode", [("flat", "refit"), ("flat", "rebuild"), ("two_level", "refit")])
@pytest.mark.parametrize("case", list(CASES))
def test_scene_equals_a_fresh_scene_of_the_host_references(instance, case, levels, mode):
    desc, v1, a, ra = run_case(instance, case, levels, mode)
    same_finite_bits(ra.read_vertices(0, len(v1)), as_rows(v1))
    b, rb = renderer(instance, with_vertices(desc, v1), levels)
    assert_same_hits(a, b, 50_000)
    assert_same_render(ra, rb)
    assert same_bits(ra.read_aov(0), rb.read_aov(0))                                               # the normal plane
    if mode == "rebuild":
        assert_same_structure(a, b)


@pytest.mark.parametrize("case", list(CASES))
def test_render_matches_the_oracle(instance, case):
    desc, v1, _, r = run_case(instance, case, "flat", "refit", size=(32, 24))
    img, _ = render(r, 5, seed=7, depth=4)
    o = OracleRenderer(OracleScene(with_vertices(desc, v1)), 32, 24)
    o.set_depth(4)
    o.set_seed(7)
    o.step(5)
    assert np.array_equal(bits(img), bits(o.read_hdr()))


# ---- 3: the reach ----------------------------------------------------------------------------------------------------------------
def test_an_update_next_to_a_set_moves_its_boundary_normals(instance):
    desc = waved_positions(sheet_scene())
    a, r = renderer(instance, desc)
    r.add_normals(N_ROOM, 400)                                                                     # the sheet's vertices 0 .. 399
    before = r.read_vertices(0, len(desc.vertices))
    v1 = desc.vertices.copy()
    v1["vv"][N_ROOM + 400:N_ROOM + 441, 1] += np.float32(0.07)                                     # 400 .. 440 alone: outside the set, inside its reach
    r.update_vertices(v1[N_ROOM + 400:N_ROOM + 441], first=N_ROOM + 400)
    got = r.read_vertices(0, len(v1))
    want = as_rows(host_normals(desc, v1, N_ROOM, 400))
    same_finite_bits(got, want)
    changed = (got.view(np.uint32) != before.view(np.uint32)).any(axis=1)
    assert changed[N_ROOM:N_ROOM + 400].any() and not changed[:N_ROOM + 330].any()                 # the boundary rows, and nothing far from them
    b, rb = renderer(instance, with_vertices(desc, as_vertices(want)))
    assert_same_hits(a, b, 20_000)
    assert_same_render(ra=r, rb=rb)


def test_an_update_outside_every_reach_runs_nothing_more(instance):
    """What says that no normal kernel ran: the span the structure is told.  In a two-level scene it is visible as meshes_touched -- the
    room's vertices belong to the cube mesh alone, and a recomputed set would add the sheet's range to the span."""
    desc = instanced_sheets(12, seed=5)
    a, r = renderer(instance, desc, "two_level")
    ns = r.add_normals(N_ROOM, 400)
    assert r.geometry_update_info().meshes_touched == 1                                            # add_normals: the sheet's range
    before = r.read_vertices(0, len(desc.vertices))
    v1 = as_vertices(before).copy()
    v1["vv"][:N_ROOM] *= np.float32(1.05)
    r.update_vertices(v1[:N_ROOM], first=0)
    u = r.geometry_update_info()
    assert (u.mode, u.meshes_touched) == (abi.GEOMETRY_REFIT, 1)
    got = r.read_vertices(0, len(v1))
    assert same_bits(got[N_ROOM:], before[N_ROOM:]) and same_bits(got[:N_ROOM], as_rows(v1)[:N_ROOM])
    v2 = v1.copy()
    v2["vv"][N_ROOM + 900:, 1] += np.float32(0.05)                                                 # the sheet's far end: past the set's reach
    r.update_vertices(v2[N_ROOM + 900:], first=N_ROOM + 900)
    assert same_bits(r.read_vertices(N_ROOM, 400), before[N_ROOM:N_ROOM + 400])
    # the control: a set that reaches into the room is recomputed by the same room update, and the span then takes in the sheet
    r.remove_normals(ns)
    r.add_normals(N_ROOM - 1, 401)
    r.update_vertices(v2[:N_ROOM], first=0)
    assert r.geometry_update_info().meshes_touched == 2
    want = host_normals(desc, v2, N_ROOM - 1, 401)
    same_finite_bits(r.read_vertices(0, len(v2)), as_rows(want))
    b, rb = renderer(instance, with_vertices(desc, want), "two_level")
    assert_same_hits(a, b, 20_000)


# ---- 4: one update of the structure a call; the bind pose stays; removal ----------------------------------------------------------
def test_one_structure_update_per_call_and_what_removal_leaves(instance):
    desc = sheet_scene()
    j, w = sheet_influences(desc.vertices)
    a, ra = renderer(instance, desc)
    skin = ra.add_skin(N_ROOM, j, w, 2)
    ns = ra.add_normals(N_ROOM, N_SHEET)
    assert ns == 0
    ra.pose({skin: bend(0.5, lift=0.05)})
    u = ra.geometry_update_info()                                                                  # ONE update of the structure
    assert (u.mode, u.meshes_touched) == (abi.GEOMETRY_REFIT, 1) and u.update_ms >= 0 and u.box_area > 0 and u.box_area_built > 0
    v1 = host_normals(desc, host_posed(desc.vertices, N_ROOM, j, w, bend(0.5, lift=0.05)), N_ROOM, N_SHEET)
    c, rc = renderer(instance, desc)
    rc.update_vertices(v1[N_ROOM:], first=N_ROOM)
    assert_same_structure(a, c)
    bones = bend(-0.3)                                                                             # a second pose starts from the bind pose
    ra.pose({skin: bones})
    posed = host_posed(desc.vertices, N_ROOM, j, w, bones)
    v2 = host_normals(desc, posed, N_ROOM, N_SHEET)
    same_finite_bits(ra.read_vertices(0, len(v2)), as_rows(v2))
    ra.remove_normals(ns)                                                                          # the vertices stay as they are
    assert same_bits(ra.read_vertices(0, len(v2)), as_rows(v2))
    assert ra.add_normals(N_ROOM, 10) == ns + 1                                                    # ids count up, never reused
    ra.remove_normals(ns + 1)
    ra.pose({skin: bones})                                                                         # and the next pose writes the skinning rule's normals again
    same_finite_bits(ra.read_vertices(0, len(v2)), as_rows(posed))
    assert not same_bits(as_rows(posed)[N_ROOM:, 3:6], as_rows(v2)[N_ROOM:, 3:6])
    b, rb = renderer(instance, with_vertices(desc, posed))
    assert_same_hits(a, b, 20_000)
    assert_same_render(ra, rb)


def test_the_timing_hook_counts_the_layouts_bytes_and_leaves_the_scene_alone(instance):
    desc = waved_positions(sheet_scene())
    _, r = renderer(instance, desc)
    ns = r.add_normals(N_ROOM, N_SHEET)
    before = r.read_vertices(0, len(desc.vertices))
    ms, nbytes = r.debug_normals_timing(ns, reps=3)
    assert ms[0] > 0 and ms[1] > 0
    faces, slices = 2 * 32 * 32, (N_SHEET + 63) // 64
    assert nbytes == (faces * (12 + 3 * 16 + 16), N_SHEET * 4 + slices * 8 + 3 * faces * (4 + 16) + N_SHEET * (32 + 12))
    assert same_bits(r.read_vertices(0, len(desc.vertices)), before)
    out = (C.c_float * 2)()
    assert abi.lib().glz_debug_normals_timing(r._h, ns + 1, 3, C.cast(out, C.c_void_p), None) == abi.E_ARG
    assert abi.lib().glz_debug_normals_timing(r._h, ns, 0, C.cast(out, C.c_void_p), None) == abi.E_ARG
    assert abi.lib().glz_debug_normals_timing(r._h, ns, 3, None, None) == abi.E_ARG


# ---- 5: refused arguments --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("levels", ["flat", "two_level"])
def test_refused_arguments_change_nothing(instance, levels):
    desc = instanced_sheets(10, seed=8)
    a, r = renderer(instance, desc, levels)
    _, ref = renderer(instance, desc, levels)
    ns = r.add_normals(N_ROOM, 500)                                                                # a set that is there
    ref.add_normals(N_ROOM, 500)
    for x in (r, ref):
        x.set_depth(4)
        x.set_seed(5)
        x.step(3)
    n_all = len(desc.vertices)
    before, v_before = structure(a), r.read_vertices(0, n_all)
    lib = abi.lib()
    labels = np.arange(100, dtype=np.uint32)
    bad_labels = labels.copy()
    bad_labels[7] = 100

    def add(first, n, groups=None):
        s = abi.Normals(first, n, None if groups is None else groups.ctypes.data)
        return lib.glz_renderer_add_normals(r._h, C.cast(C.byref(s), C.c_void_p))

    far = N_ROOM + 600                                                                             # clear of the set that is there
    assert lib.glz_renderer_add_normals(r._h, None) == abi.E_ARG                                   # a null pointer
    assert add(far, 0) == abi.E_ARG                                                                # none
    assert add(n_all - 99, 100) == abi.E_ARG and add(0xFFFFFFFF, 2) == abi.E_ARG                   # past the end (and a sum that wraps)
    assert add(far, 100, bad_labels) == abi.E_ARG                                                  # a label >= n_vertices
    assert add(N_ROOM + 499, 10) == abi.E_ARG and add(0, N_ROOM + 1) == abi.E_ARG                  # overlaps, at either end
    assert add(N_ROOM, 500) == abi.E_ARG
    assert lib.glz_renderer_remove_normals(r._h, ns + 1) == abi.E_ARG and lib.glz_renderer_remove_normals(r._h, -1) == abi.E_ARG
    with pytest.raises(ValueError):
        r.add_normals(far, 100, labels[:99])
    with pytest.raises(ValueError):
        r.add_normals(far, 100, "welded")
    with pytest.raises(glaze_amd.GlazeError):
        r.add_normals(far, 100, bad_labels)
    assert_same_bytes(before, structure(a))
    assert same_bits(r.read_vertices(0, n_all), v_before)
    for x in (r, ref):
        x.step(4)
    assert np.array_equal(bits(r.read_hdr()), bits(ref.read_hdr()))                                # the accumulation went on, on the same scene
    assert np.array_equal(bits(r.read_result()), bits(ref.read_result()))
    assert add(far, 100, labels) == ns + 1                                                         # (and one that is fine)


def test_weld_takes_the_labels_from_the_devices_vertices(instance):
    """groups="weld": a sheet whose first and last columns are one seam (the same positions and normals, other texture coordinates)"""
    v, idx = sheet(8)
    v["vv"][:, 1] += (0.1 * np.sin(7.0 * v["vv"][:, 0])).astype(np.float32)
    v["vv"][72:81] = v["vv"][0:9]                                                                  # the last row of vertices on top of the first
    desc = room_with(v, idx)
    _, r = renderer(instance, desc)
    r.add_normals(N_ROOM, 81, groups="weld")
    labels = glaze_amd.host_weld_groups(desc.vertices[N_ROOM:])
    assert np.array_equal(labels[72:81], np.arange(9)) and np.array_equal(labels[:72], np.arange(72))
    got = r.read_vertices(N_ROOM, 81)
    same_finite_bits(got, as_rows(host_normals(desc, desc.vertices, N_ROOM, 81, labels))[N_ROOM:])
    assert same_bits(got[72:81, 3:6], got[0:9, 3:6]) and not same_bits(got[72:81, 6:8], got[0:9, 6:8])


# ---- 6: the other devices of set_devices ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("devices_first", [True, False])
def test_loopback_devices_follow_a_normal_set(instance, loopback, devices_first):
    desc = instanced_sheets(10, seed=9)
    j, w = sheet_influences(desc.vertices)
    bones = bend(0.45)
    r = glaze_amd.RayTraceRenderer.new(instance, make_scene(instance, desc, "flat"), 136, 200)
    if devices_first:
        r.set_devices([instance.device] * 2)
    skin = r.add_skin(N_ROOM, j, w, 2)
    r.add_normals(N_ROOM, N_SHEET)
    r.pose({skin: bend(-0.2)})
    if not devices_first:
        r.set_devices([instance.device] * 2)                                                       # the replica is made of the posed scene, sets included
    r.pose({skin: bones})
    v1 = host_normals(desc, host_posed(desc.vertices, N_ROOM, j, w, bones), N_ROOM, N_SHEET)
    one = glaze_amd.RayTraceRenderer.new(instance, make_scene(instance, with_vertices(desc, v1), "flat"), 136, 200)
    assert_same_render(r, one)
    assert np.array_equal(r.read_rgba8(), one.read_rgba8())
