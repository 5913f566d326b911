"""The host rule for the instance boxes of a two-level top level (glz_host_instance_boxes), on the CPU.

A box must hold every world vertex the tracer computes for its instance (single precision, four rounded terms), whatever the
transform; non-finite transforms give the padded box around the origin; past the exact-box budget the remaining instances, in
instance order, take the corners of their mesh's box.  The device kernel of update_transforms is held to this rule bit for bit
(tests/test_gpu_transform_update.py).
"""
import numpy as np
import pytest

import glaze_amd
from glaze_amd.scene_desc import INSTANCE_DTYPE, MESH_DTYPE, VERTEX_DTYPE, SceneDesc


def random_desc(seed, n_meshes=3, n_instances=40, non_finite=()):
    rng = np.random.default_rng(seed)
    verts, idx, meshes = [], [], []
    for m in range(n_meshes):
        nv = int(rng.integers(3, 60))
        p = rng.normal(0, 1, (nv, 3)) * rng.uniform(0.1, 20, 3) + rng.uniform(-50, 50, 3)
        base = len(verts)
        verts += [tuple(x) for x in p]
        tri = rng.integers(0, nv, (int(rng.integers(1, 40)), 3)) + base
        mesh = np.zeros(1, MESH_DTYPE)[0]
        mesh["id"], mesh["index_offset"], mesh["index_count"], mesh["material"] = m, len(idx), tri.size, 0
        meshes.append(mesh)
        idx += tri.reshape(-1).tolist()
    v = np.zeros(len(verts), VERTEX_DTYPE)
    v["vv"] = np.asarray(verts, np.float32)
    mats = []
    for i in range(n_instances):
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        m = np.eye(4)
        m[:3, :3] = q @ np.diag(rng.uniform(0.01, 30, 3) * np.where(rng.random(3) < 0.3, -1.0, 1.0))
        m[:3, 3] = rng.uniform(-1e3, 1e3, 3)
        if i % 7 == 3:
            m = np.eye(4)
        mats.append(np.asarray(m, np.float32).T.reshape(16))
    t = np.stack(mats)
    for i, kind in non_finite:
        t[i] = kind
    inst = np.array([(int(rng.integers(0, n_meshes)), i) for i in range(n_instances)] + [(999, 0)], INSTANCE_DTYPE)   # + one dangling
    return SceneDesc(v, np.asarray(idx, np.uint32), np.array(meshes, MESH_DTYPE), t, inst)


def world_points(desc, mesh_id, t):
    """the tracer's world vertices (device/math.h xform_point): float32, m0 x + m4 y + m8 z + m12, left to right"""
    m = desc.meshes[mesh_id]
    ids = np.unique(desc.indices[m["index_offset"]:m["index_offset"] + m["index_count"]])
    p = desc.vertices["vv"][ids].astype(np.float32)
    M = desc.transforms[t]
    with np.errstate(all="ignore"):
        return np.stack([((M[k] * p[:, 0] + M[4 + k] * p[:, 1]) + M[8 + k] * p[:, 2]) + M[12 + k] for k in range(3)], 1)


def origin_box():
    pad = np.float64(1e-5 * 1e-3)
    return (np.nextafter(np.float32(-pad), np.float32(-np.inf)), np.nextafter(np.float32(pad), np.float32(np.inf)))


@pytest.mark.parametrize("seed", range(6))
def test_every_world_vertex_lies_inside_its_instance_box(seed):
    desc = random_desc(seed)
    lo, hi = glaze_amd.host_instance_boxes(desc)
    assert lo.shape == (desc.instances.shape[0] - 1, 4)                                         # the dangling instance is dropped
    assert (lo[:, 3] == 0).all() and (hi[:, 3] == 0).all()
    for i, (mesh_id, t) in enumerate(desc.instances[:-1].tolist()):
        w = world_points(desc, mesh_id, t).astype(np.float64)
        assert (lo[i, :3].astype(np.float64) <= w).all() and (w <= hi[i, :3].astype(np.float64)).all(), i
        assert (lo[i, :3] < hi[i, :3]).all()


def test_non_finite_transforms_give_the_padded_box_around_the_origin():
    nan_t = np.full(16, np.nan, np.float32)
    nan_move = np.eye(4, dtype=np.float32).reshape(16).copy()
    nan_move[12:15] = np.nan                                                                   # every world coordinate is NaN
    desc = random_desc(11, non_finite=((0, nan_t), (5, nan_move)))
    lo, hi = glaze_amd.host_instance_boxes(desc)
    l, h = origin_box()
    for i in (0, 5):
        assert (lo[i, :3] == l).all() and (hi[i, :3] == h).all(), i
    inf_t = np.eye(4, dtype=np.float32).reshape(16).copy()
    inf_t[12] = np.inf
    desc = random_desc(12, non_finite=((2, inf_t),))
    lo, hi = glaze_amd.host_instance_boxes(desc)
    assert lo[2, 0] == -np.inf and hi[2, 0] == np.inf                                          # x is +inf everywhere: the whole axis
    w = world_points(desc, desc.instances[2][0], 2)
    assert (lo[2, 1:3] <= w[:, 1:3]).all() and (w[:, 1:3] <= hi[2, 1:3]).all()


def test_corner_fallback_starts_where_the_budget_runs_out():
    desc = random_desc(5, n_meshes=3, n_instances=60)
    exact_lo, exact_hi = glaze_amd.host_instance_boxes(desc)
    counts = []
    for m in desc.meshes:
        counts.append(np.unique(desc.indices[m["index_offset"]:m["index_offset"] + m["index_count"]]).size)
    budget = sum(counts[mi] for mi, _ in desc.instances[:20].tolist()) + 1                     # runs out a third of the way
    lo, hi = glaze_amd.host_instance_boxes(desc, budget=budget)
    spent, fell_back = 0, []
    for i, (mi, _) in enumerate(desc.instances[:-1].tolist()):
        if spent + counts[mi] <= budget:
            spent += counts[mi]
            assert np.array_equal(lo[i].view(np.uint32), exact_lo[i].view(np.uint32)), i
            assert np.array_equal(hi[i].view(np.uint32), exact_hi[i].view(np.uint32)), i
        else:
            fell_back.append(i)
            assert (lo[i] <= exact_lo[i]).all() and (exact_hi[i] <= hi[i]).all(), i           # the corners' box holds the exact one
    assert fell_back and fell_back[0] >= 20
    assert any((lo[i, :3] < exact_lo[i, :3]).any() for i in fell_back)                        # and is wider for rotated instances
    for i in fell_back:                                                                       # the corners of the mesh's vertex box
        mi, t = desc.instances[i].tolist()
        m = desc.meshes[mi]
        p = desc.vertices["vv"][desc.indices[m["index_offset"]:m["index_offset"] + m["index_count"]]]
        a, b = p.min(0), p.max(0)
        c = np.array([[(b if (k >> j) & 1 else a)[j] for j in range(3)] for k in range(8)], np.float64)
        M = desc.transforms[t].astype(np.float64).reshape(4, 4).T
        w = c @ M[:3, :3].T + M[:3, 3]
        assert (lo[i, :3] <= w.min(0)).all() and (w.max(0) <= hi[i, :3]).all(), i


def test_the_rule_is_deterministic():
    desc = random_desc(9, n_instances=200)
    a = glaze_amd.host_instance_boxes(desc)
    b = glaze_amd.host_instance_boxes(desc.copy())
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
