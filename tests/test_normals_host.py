"""The normal rule on the host (glz_host_vertex_normals: the reference k_face_vectors and k_vertex_normals must match bit for bit) against
the specification in include/glaze_abi.h ("THE NORMAL RULE"), restated here in numpy float32 with the operations in the specification's
order, and against closed forms where there is one.  glz_host_vertex_normals runs through the layout packer the device path uses, so these
cases hold the packer (faces, rows, groups) to the rule as well.  No device."""
import ctypes as C

import numpy as np
import pytest

import glaze_amd
from glaze_amd import abi
from glaze_amd.scene_desc import MESH_DTYPE, VERTEX_DTYPE
from glaze_amd.scenes import cube_scene

from test_gpu_skin import same_finite_bits
from test_gpu_vertex_update import N_ROOM, sheet, sheet_scene, waved

U = 2.0 ** -24          # the unit roundoff of float32
F32 = np.float32


def rows_of(vertices):
    return np.ascontiguousarray(vertices).view(np.float32).reshape(-1, 8)


def faces_of(indices, meshes, first, n):
    """the set's faces: the triangles of the meshes in array order, k < index_count / 3, with a corner in [first, first + n)"""
    out = []
    for m in meshes:
        off, cnt = int(m["index_offset"]), int(m["index_count"])
        tri = np.asarray(indices[off:off + 3 * (cnt // 3)], np.int64).reshape(-1, 3)
        out.append(tri[((tri >= first) & (tri < first + n)).any(axis=1)])
    return np.concatenate(out) if out else np.zeros((0, 3), np.int64)


def restate(vertices, indices, meshes, first, n, groups=None):
    """the rule, operation by operation: numpy rounds every elementwise + - * of float32 arrays to float32, and float32 sqrt and division
    are correctly rounded.  Returns (the range's vertices with the rule's normals, the faces, the face list of every vertex)."""
    v = rows_of(vertices)
    faces = faces_of(indices, meshes, first, n)
    labels = np.arange(n) if groups is None else np.asarray(groups, np.int64)
    with np.errstate(all="ignore"):
        p0, p1, p2 = (v[faces[:, c], 0:3] for c in range(3))
        a, b = p1 - p0, p2 - p0
        F = np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], -1)
        assert F.dtype == np.float32
        of_group = [[] for _ in range(n)]
        for f, tri in enumerate(faces):                                          # ascending faces, each once a group
            for c in tri:
                if first <= c < first + n and (not of_group[labels[c - first]] or of_group[labels[c - first]][-1] != f):
                    of_group[labels[c - first]].append(f)
        out = v[first:first + n].copy()
        for i in range(n):
            mine = of_group[labels[i]]
            if not mine:
                continue
            S = np.zeros(3, np.float32)
            for f in mine:
                S = S + F[f]
            d = (S[0] * S[0] + S[1] * S[1]) + S[2] * S[2]
            if d > 0 and d < np.inf:
                inv = F32(1.0) / np.sqrt(d)
                assert inv.dtype == np.float32
                S = S * inv
            out[i, 3:6] = S
    return out, faces, [of_group[labels[i]] for i in range(n)]


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


def check(vertices, indices, meshes, first, n, groups=None):
    got = glaze_amd.host_vertex_normals(vertices, indices, meshes, first, n, groups)
    want, faces, lists = restate(vertices, indices, meshes, first, n, groups)
    same_finite_bits(got, want)
    v = rows_of(vertices)[first:first + n]
    assert same_bits(got[:, 0:3], v[:, 0:3]) and same_bits(got[:, 6:8], v[:, 6:8])                # position and uv: never touched
    return got, faces, lists


def soup(rng, n_vertices=200, n_triangles=500):
    """random triangles under three meshes, two of which share an index range: their triangles count twice"""
    v = rng.normal(size=(n_vertices, 8)).astype(np.float32)
    idx = rng.integers(0, n_vertices, 3 * n_triangles).astype(np.uint32)
    meshes = np.array([(0, 0, 0, 900), (1, 0, 900, 600), (2, 0, 0, 900)], MESH_DTYPE)
    return v, idx, meshes


def one_mesh(idx):
    return np.array([(0, 0, 0, len(idx))], MESH_DTYPE)


# ---- the rule, bit for bit -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_random_soups_equal_the_restated_rule(seed):
    rng = np.random.default_rng(seed)
    v, idx, meshes = soup(rng)
    got, faces, lists = check(v, idx, meshes, 0, 200)
    assert len(faces) == 800                                                                        # 300 + 200 + 300: the shared range twice
    assert max(len(x) for x in lists) > 6 and not same_bits(got[:, 3:6], v[:, 3:6])
    check(v, idx, meshes, 37, 100)                                                                  # corners outside the range
    check(v, idx, meshes, 199, 1)
    check(v, idx, meshes, 0, 65)                                                                    # one full slice and one lane


@pytest.mark.parametrize("seed", [3, 4])
def test_random_groups_equal_the_restated_rule(seed):
    rng = np.random.default_rng(seed)
    v, idx, meshes = soup(rng)
    for first, n in ((0, 200), (50, 130)):
        groups = rng.integers(0, n, n).astype(np.uint32)
        groups[rng.random(n) < 0.5] = rng.integers(0, 8)                                            # one large group among small ones
        got, _, lists = check(v, idx, meshes, first, n, groups)
        for g in np.unique(groups):
            members = np.flatnonzero(groups == g)
            if lists[members[0]]:
                assert all(same_bits(got[m, 3:6], got[members[0], 3:6]) for m in members)           # one normal a group


def test_waved_sheet_equals_the_restated_rule():
    v, idx = sheet(32)
    v = waved(v, first=0)
    got, _, lists = check(v, idx, one_mesh(idx), 0, len(v))
    assert sorted(set(len(x) for x in lists)) == [1, 2, 3, 6]                                       # corners, edges, the inside
    exact = rows_of(v)[:, 3:6]                                                                      # (and it is the wave's normal, roughly)
    assert np.abs(got[:, 3:6] - exact).max() < 0.2 and np.allclose(np.linalg.norm(got[:, 3:6].astype(np.float64), axis=1), 1.0, atol=4 * U)
    rng = np.random.default_rng(5)
    check(v, idx, one_mesh(idx), 0, len(v), rng.integers(0, len(v), len(v)).astype(np.uint32))
    check(v, idx, one_mesh(idx), 500, 300)


def test_flat_sheet_closed_form():
    """every face vector of the flat sheet is (+0, dz * dx, +0): the sum's direction is exact, and four correctly rounded operations
    follow it -- d, sqrtf, the reciprocal, the product -- each at most 2^-24 relative"""
    v, idx = sheet(32)
    got = glaze_amd.host_vertex_normals(v, idx, one_mesh(idx), 0, len(v))
    assert not got[:, [3, 5]].view(np.uint32).any()                                                 # x and z: exactly +0
    assert np.abs(got[:, 4].astype(np.float64) - 1.0).max() <= 4 * U
    assert same_bits(got[:, 4], restate(v, idx, one_mesh(idx), 0, len(v))[0][:, 4])


# ---- groups: hard edges and seams ------------------------------------------------------------------------------------------------
def test_room_cube_welded_by_position_and_normal_keeps_its_hard_edges():
    d = cube_scene()
    v = rows_of(d.vertices)
    labels = glaze_amd.host_weld_groups(d.vertices)
    assert labels.dtype == np.uint32 and np.array_equal(labels, np.arange(24))                      # the normals differ: nothing welds
    got, _, lists = check(d.vertices, d.indices, d.meshes, 0, 24, labels)
    assert all(1 <= len(x) <= 2 for x in lists)
    axis = np.abs(v[:, 3:6]).argmax(axis=1)
    for i in range(24):                                                                             # on its face's axis, whichever way the winding points
        others = [k for k in range(3) if k != axis[i]]
        assert not got[i, 3:6][others].any() and abs(abs(float(got[i, 3 + axis[i]])) - 1.0) <= 4 * U


def test_room_cube_grouped_by_position_gets_corner_normals():
    d = cube_scene()
    v = rows_of(d.vertices)
    labels = np.array([min(j for j in range(24) if same_bits(v[j, 0:3], v[i, 0:3])) for i in range(24)], np.uint32)
    assert len(np.unique(labels)) == 8 and all((labels == g).sum() == 3 for g in np.unique(labels))
    got, faces, lists = check(d.vertices, d.indices, d.meshes, 0, 24, labels)
    for g in np.unique(labels):
        members = np.flatnonzero(labels == g)
        assert same_bits(got[members[1], 3:6], got[members[0], 3:6]) and same_bits(got[members[2], 3:6], got[members[0], 3:6])
        touched = {tuple(np.abs(v[c, 3:6]).argmax() for c in faces[f])[0] for f in lists[members[0]]}
        assert touched == {0, 1, 2}                                                                 # the three cube faces that meet there
        assert (got[members[0], 3:6] != 0).all()


def seam_strip(columns=12):
    """two rows around a cylinder; the last column repeats the first one's positions and normals under other texture coordinates"""
    k = np.arange(columns + 1)
    ang = (2.0 * np.pi * (k % columns) / columns)
    ring = np.stack([np.cos(ang), np.zeros_like(ang), np.sin(ang)], -1).astype(np.float32)
    v = np.zeros((2, columns + 1), VERTEX_DTYPE)
    for r in range(2):
        v["vv"][r] = ring + np.array([0, r, 0], np.float32)
        v["vn"][r] = ring
        v["vt"][r] = np.stack([k / columns, np.full(columns + 1, float(r))], -1)
    idx = np.arange(2 * (columns + 1), dtype=np.uint32).reshape(2, columns + 1)
    a, b, c, e = idx[0, :-1], idx[0, 1:], idx[1, 1:], idx[1, :-1]
    return v.reshape(-1), np.stack([a, b, c, a, c, e], -1).reshape(-1)


def test_a_seam_is_smooth_when_welded_and_not_otherwise():
    v, idx = seam_strip()
    n, last = len(v), 12
    rows = rows_of(v)
    assert same_bits(rows[0, 0:6], rows[last, 0:6]) and not same_bits(rows[0, 6:8], rows[last, 6:8])
    labels = glaze_amd.host_weld_groups(v)
    want = np.arange(n, dtype=np.uint32)
    want[last], want[2 * last + 1] = 0, last + 1
    assert np.array_equal(labels, want)
    welded, _, _ = check(v, idx, one_mesh(idx), 0, n, labels)
    alone, _, _ = check(v, idx, one_mesh(idx), 0, n)
    for first_col, last_col in ((0, last), (last + 1, 2 * last + 1)):
        assert same_bits(welded[first_col, 3:6], welded[last_col, 3:6])
        assert not same_bits(alone[first_col, 3:6], alone[last_col, 3:6])
        assert not same_bits(welded[first_col, 6:8], welded[last_col, 6:8])
    inner = [i for i in range(n) if i not in (0, last, last + 1, 2 * last + 1)]
    assert same_bits(welded[inner], alone[inner])                                                   # away from the seam nothing changes


def test_weld_labels_tell_signed_zeros_apart_and_take_the_lowest_index():
    v = np.zeros((5, 8), np.float32)
    v[:, 4] = 1.0
    v[1, 0] = -0.0                                                                                  # -0 is not +0
    v[3, 7] = 9.0                                                                                   # texture coordinates do not count
    v[4, 4] = 2.0
    assert glaze_amd.host_weld_groups(v).tolist() == [0, 1, 0, 0, 4]
    assert glaze_amd.host_weld_groups(np.zeros((0, 8), np.float32)).tolist() == []


# ---- specific cases ---------------------------------------------------------------------------------------------------------------
def fan_case():
    """six vertices: a fan of three triangles around vertex 0, vertex 5 in no face"""
    v = np.zeros((6, 8), np.float32)
    v[:, 0:3] = [(0, 0, 0), (1, 0, 0), (0.5, 0.2, 1), (-1, 0.1, 0.5), (-0.5, 0, -1), (3, 3, 3)]
    v[:, 3:6] = (0.6, 0.0, 0.8)
    v[:, 6:8] = np.arange(12).reshape(6, 2)
    return v, np.array([0, 1, 2, 0, 2, 3, 0, 3, 4], np.uint32)


def test_a_vertex_without_a_face_keeps_its_bits():
    v, idx = fan_case()
    v[5, 3:6] = (np.nan, -0.0, 1e-42)                                                               # whatever bits it has
    got, _, lists = check(v, idx, one_mesh(idx), 0, 6)
    assert lists[5] == [] and np.array_equal(got[5].view(np.uint32), v[5].view(np.uint32))
    assert not same_bits(got[:5, 3:6], v[:5, 3:6])


def test_a_vertex_of_zero_area_faces_alone_comes_out_as_the_zero_sum():
    v, _ = fan_case()
    v[2, 0:3] = v[1, 0:3]                                                                           # two corners in one place
    idx = np.array([0, 1, 2, 1, 2, 2, 3, 3, 3], np.uint32)                                          # and corners named twice
    got, _, lists = check(v, idx, one_mesh(idx), 0, 6)
    assert lists[1] == [0, 1] and not got[:4, 3:6].view(np.uint32).any()                            # S itself: +0, not normalised, no NaN


def test_a_nan_position_reaches_exactly_the_normals_whose_groups_touch_it():
    v, idx = sheet(8)
    v = rows_of(waved(v, first=0)).copy()
    bad = 40
    v[bad, 1] = np.nan
    for groups in (None, np.where(np.arange(81) % 9 == 0, 0, np.arange(81)).astype(np.uint32)):    # alone, and with one column in a group
        got, faces, lists = check(v, idx, one_mesh(idx), 0, 81, groups)
        touched = np.array([any(bad in faces[f] for f in lists[i]) for i in range(81)])
        assert 6 <= touched.sum() < 81
        assert np.array_equal(~np.isfinite(got[:, 3:6]).all(axis=1), touched)
    v[bad, 1] = np.inf
    check(v, idx, one_mesh(idx), 0, 81)


def test_a_corner_outside_the_range_is_read_and_never_written_and_out_may_be_the_input():
    d = sheet_scene()
    v = rows_of(waved(d.vertices)).copy()
    first, n = N_ROOM + 200, 400
    got, faces, _ = check(v, d.indices, d.meshes, first, n)
    assert (faces < first).any() and (faces >= first + n).any()
    moved = v.copy()
    moved[first - 1, 0:3] += 0.05                                                                   # a neighbour outside moves: the boundary normals follow
    assert not same_bits(glaze_amd.host_vertex_normals(moved, d.indices, d.meshes, first, n), got)
    inplace = v.copy()
    idx = np.ascontiguousarray(d.indices, np.uint32)
    meshes = np.ascontiguousarray(d.meshes, MESH_DTYPE)
    rc = abi.lib().glz_host_vertex_normals(inplace.ctypes.data, len(inplace), idx.ctypes.data, len(idx), meshes.ctypes.data, len(meshes), first, n, None,
                                           inplace[first:].ctypes.data)
    assert rc == 0
    assert same_bits(inplace[first:first + n], got)
    assert same_bits(inplace[:first], v[:first]) and same_bits(inplace[first + n:], v[first + n:])


def test_refused_arguments():
    v, idx = fan_case()
    meshes = one_mesh(idx)
    out = np.zeros((6, 8), np.float32)
    call = abi.lib().glz_host_vertex_normals

    def run(vertices=v, n_vertices=6, indices=idx, n_indices=9, m=meshes, first=0, n=6, groups=None, o=out):
        return call(None if vertices is None else vertices.ctypes.data, n_vertices, None if indices is None else indices.ctypes.data, n_indices, m.ctypes.data, len(m),
                    first, n, None if groups is None else groups.ctypes.data, None if o is None else o.ctypes.data)

    assert run() == 0
    assert run(vertices=None) == abi.E_ARG and run(o=None) == abi.E_ARG and run(indices=None) == abi.E_ARG   # null pointers
    assert run(n=0) == abi.E_ARG                                                                    # none
    assert run(first=1) == abi.E_ARG and run(first=0xFFFFFFFF, n=2) == abi.E_ARG                    # past the end (and a sum that wraps)
    assert run(groups=np.array([0, 1, 2, 3, 4, 6], np.uint32)) == abi.E_ARG                         # a label >= n
    assert run(first=2, n=3, groups=np.array([0, 3, 1], np.uint32)) == abi.E_ARG                    # (>= n, not >= the vertex count)
    assert run(first=2, n=3, groups=np.array([0, 2, 1], np.uint32)) == 0
    assert run(n_indices=8) == abi.E_ARG                                                            # a mesh past the indices
    assert run(n_vertices=4, n=4) == abi.E_ARG                                                      # an index >= the vertex count
    with pytest.raises(ValueError):
        glaze_amd.host_vertex_normals(v, idx, meshes, 0, 6, groups=np.zeros(5, np.uint32))
    with pytest.raises(glaze_amd.GlazeError):
        glaze_amd.host_vertex_normals(v, idx, meshes, 0, 6, groups=np.full(6, 6, np.uint32))
    assert abi.lib().glz_host_weld_groups(None, 3, out.ctypes.data) == abi.E_ARG and abi.lib().glz_host_weld_groups(v.ctypes.data, 3, None) == abi.E_ARG
