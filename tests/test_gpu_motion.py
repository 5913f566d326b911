"""Motion vectors and history reprojection on the device (glz_renderer_read_motion, glz_renderer_reproject; include/glaze_abi.h holds the
specification).  The motion plane must equal a float64 restatement on the oracle's hits within a bound derived from the operation count;
two closed forms pin the geometry down; the device kernels must equal the host references bit for bit (the host references are checked
against float64 in tests/test_reproject_host.py); none of it may disturb a running accumulation."""
import ctypes as C

import numpy as np
import pytest

import glaze_amd
from glaze_amd import abi
from glaze_amd.scene_desc import INSTANCE_DTYPE, SceneDesc, _clone, make_camera, make_light, make_material, make_meta
from glaze_amd.scenes import _Builder, atrium_scene, cube_scene, forest_scene, mirror_room_scene
from oracle.pyoracle import OracleScene

from denoise_ref import synthetic_frame
from reproject_ref import REPROJECT_CASES, bits, cameras, projection_bounds, projection_points, reference_project, reproject_inputs

pytestmark = pytest.mark.gpu

W, H = 128, 72
MISS = 0xFFFFFFFF


def make_scene(instance, desc, levels="auto"):
    instance.set_as_levels(levels)
    try:
        scene = glaze_amd.RayTraceScene.from_desc(instance, desc)
    finally:
        instance.set_as_levels("auto")
    if levels != "auto":
        assert scene.info().as_levels == (2 if levels == "two_level" else 1)
    return scene


def moved_camera(cam, shift=(0.45, 0.1, -0.4), turn=(0.6, -0.2, 0.5)):
    """the camera about 0.6 m away and turned"""
    c = _clone(cam)
    c.position[:] = [a + b for a, b in zip(cam.position[:], shift)]
    c.target[:] = [a + b for a, b in zip(cam.target[:], turn)]
    return c


def moved_transforms(transforms, seed, every=1):
    """every `every`-th transform (transform 0 included) turned about y by up to 0.2 rad and shifted by up to 0.3 m: (n, 16) float32"""
    rng = np.random.default_rng(seed)
    out = []
    for i, t in enumerate(np.asarray(transforms, np.float64).reshape(-1, 16)):
        m = t.reshape(4, 4).T
        if i % every == 0:
            a = rng.uniform(-0.2, 0.2)
            d = np.eye(4)
            d[:3, :3] = [[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]
            d[:3, 3] = rng.uniform(-0.3, 0.3, 3)
            m = d @ m
        out.append(m.T.reshape(16))
    return np.asarray(out, np.float32)


def oracle_hits(desc, ren):
    """the oracle's closest hits of the centre rays the device generates (as test_first_hit_pass_equals_the_oracle)"""
    o, d = ren.debug_camera_rays((0.5, 0.5))
    return OracleScene(desc).trace_closest(o.reshape(-1, 3), d.reshape(-1, 3), tmin=1e-4)


def restate_motion(desc, hits, prev_camera, prev_transforms, w, h):
    """float64 motion plane on the oracle's hits: vertex positions from the scene description, barycentrics from the oracle, the previous
    matrices in float64, host_project_constants' rounded matrices.  Returns the plane (n x 3), the hit and valid masks, the instance
    words and the three bounds of the issue (dfx, dfy, dz' / z')."""
    t, tri, inst, u, v = hits
    hit = np.isfinite(t)
    meshes = {int(m["id"]): m for m in desc.meshes}
    inst_mesh = [meshes[int(i["mesh_id"])] for i in desc.instances]
    counts = np.array([int(m["index_count"]) // 3 for m in inst_mesh], np.int64)
    base = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    ii = np.where(hit, inst, 0).astype(np.int64)
    local = np.where(hit, tri.astype(np.int64) - base[ii], 0)
    assert (local >= 0).all() and (local[hit] < counts[ii][hit]).all()
    first = np.array([int(m["index_offset"]) for m in inst_mesh], np.int64)[ii] + 3 * local
    vid = np.stack([desc.indices[first + k] for k in range(3)], -1)
    xf_id = np.array([int(i["transform_id"]) for i in desc.instances], np.int64)[ii]
    vv = desc.vertices["vv"][vid].astype(np.float64)                                   # n x 3 x 3
    b1, b2 = u.astype(np.float64), v.astype(np.float64)
    b0 = 1.0 - b1 - b2
    p_obj = vv[:, 0] * b0[:, None] + vv[:, 1] * b1[:, None] + vv[:, 2] * b2[:, None]
    M = np.asarray(prev_transforms, np.float64).reshape(-1, 4, 4).transpose(0, 2, 1)[xf_id]
    p_prev = np.einsum("nij,nj->ni", M[:, :3, :3], p_obj) + M[:, :3, 3]
    persp = prev_camera.type == abi.CAMERA_PERSPECTIVE
    w2c, c2s = glaze_amd.host_project_constants(prev_camera, w, h)
    proj, valid, z_c = reference_project(w2c, c2s, persp, w, h, p_prev)
    valid &= hit
    py, px = np.divmod(np.arange(w * h), w)
    plane = np.stack([proj[:, 0] - (px + 0.5), proj[:, 1] - (py + 0.5), proj[:, 2]], -1)
    plane[~valid] = (0.0, 0.0, np.inf)
    with np.errstate(all="ignore"):
        bounds = projection_bounds(c2s, persp, w, h, p_prev, prev_camera.position[:], z_c, proj[:, 2])
    words = np.where(hit, inst, np.uint32(MISS)).astype(np.uint32)
    return plane, hit, valid, words, bounds


def check_motion(name, got, restated):
    """instance bits and the miss / invalid sets identical, the three coordinates within the bounds; returns the largest error / bound"""
    plane, hit, valid, words, (bx, by, bz) = restated
    got = got.reshape(-1, 4)
    assert np.array_equal(bits(got[:, 3]), words), name
    got_valid = np.isfinite(got[:, 2])
    assert np.array_equal(got_valid, valid), "%s: %d pixels differ in validity" % (name, (got_valid != valid).sum())
    assert (got[~valid, :2] == 0).all() and np.isposinf(got[~valid, 2]).all()
    g = got[valid].astype(np.float64)
    ex, ey = np.abs(g[:, 0] - plane[valid, 0]) / bx[valid], np.abs(g[:, 1] - plane[valid, 1]) / by[valid]
    ez = np.abs(g[:, 2] - plane[valid, 2]) / plane[valid, 2] / bz[valid]
    worst = max(ex.max(), ey.max(), ez.max())
    print("%s: %d hits, %d valid; largest error as a fraction of its bound: fx %.3f, fy %.3f, z' %.3f" % (name, hit.sum(), valid.sum(), ex.max(), ey.max(), ez.max()))
    assert worst <= 1.0, name
    return worst


# ---------------------------------------------------------------------------------------------------------------------
# 5. the motion plane equals a float64 restatement on the oracle's hits
# ---------------------------------------------------------------------------------------------------------------------
def motion_scenes():
    ortho_cube = cube_scene()
    ortho_cube.camera = make_camera(position=(0.1, 0.15, -0.2), target=(0.3, 0.05, 1.0), near=1e-3, far=100.0, orthographic=True, scale=1.0)
    return {"forest, flattened": (lambda: forest_scene(40), "flat"), "forest, two levels": (lambda: forest_scene(40), "two_level"),
            "room": (lambda: mirror_room_scene(mirror=False), "auto"), "cube, orthographic": (lambda: ortho_cube, "auto")}


@pytest.mark.parametrize("name", list(motion_scenes()))
def test_motion_plane_equals_float64_on_the_oracles_hits(instance, name):
    make, levels = motion_scenes()[name]
    desc = make()
    ren = glaze_amd.RayTraceRenderer.new(instance, make_scene(instance, desc, levels), W, H)
    hits = oracle_hits(desc, ren)
    assert np.isfinite(hits[0]).sum() > 1000
    prev_cam = moved_camera(desc.camera, shift=(0.05, 0.02, -0.04), turn=(0.05, -0.02, 0.0)) if "orthographic" in name else moved_camera(desc.camera)
    prev_xf = moved_transforms(desc.transforms, seed=4, every=1 if name == "room" else 3)
    assert not np.array_equal(prev_xf[0], desc.transforms[0])
    # the previous camera moved and turned, previous transforms given
    check_motion(name + ", camera and instances moved", ren.read_motion(prev_cam, prev_xf), restate_motion(desc, hits, prev_cam, prev_xf, W, H))
    # previous transforms NULL: the scene's own
    moved = ren.read_motion(prev_cam)
    check_motion(name + ", camera moved", moved, restate_motion(desc, hits, prev_cam, desc.transforms, W, H))
    assert np.array_equal(bits(moved), bits(ren.read_motion(prev_cam, desc.transforms)))
    # static: the previous state is the current one
    static = ren.read_motion(desc.camera)
    restated = restate_motion(desc, hits, desc.camera, desc.transforms, W, H)
    check_motion(name + ", static", static, restated)
    _, hit, valid, _, (bx, by, bz) = restated
    assert np.array_equal(valid, hit)                                                  # what the camera sees projects
    s = static.reshape(-1, 4)[valid].astype(np.float64)
    depth = ren.read_aov(0).reshape(-1, 4)[valid, 3].astype(np.float64)
    print("  static: largest |motion| %.3g px (%.3f of its bound), z' against read_aov's depth %.3f of its bound" % (
        np.abs(s[:, :2]).max(), max((np.abs(s[:, 0]) / bx[valid]).max(), (np.abs(s[:, 1]) / by[valid]).max()), (np.abs(s[:, 2] - depth) / depth / bz[valid]).max()))
    assert (np.abs(s[:, 0]) <= bx[valid]).all() and (np.abs(s[:, 1]) <= by[valid]).all()
    assert (np.abs(s[:, 2] - depth) / depth <= bz[valid]).all()


# ---------------------------------------------------------------------------------------------------------------------
# 6. closed forms: a wall that fills the view and a card in front of it, a perspective camera looking down -z
# ---------------------------------------------------------------------------------------------------------------------
D1, D2 = 4.0, 8.0
FOVX = np.float32(np.radians(np.float32(70.0)))


def wall_and_card():
    B = _Builder()
    B.grid((-12, -8, -D2), (24, 0, 0), (0, 16, 0), 2, 2, 1)                           # the wall (+z), instance 0 under transform 0
    B.grid((-0.9, -0.6, -D1), (1.8, 0, 0), (0, 1.2, 0), 1, 1, 1)                      # the card, instance 1 under transform 1
    vertices, indices, meshes = B.finish()
    transforms = np.stack([np.eye(4, dtype=np.float32).reshape(16)] * 2)
    camera = make_camera(position=(0, 0, 0), target=(0, 0, -100), up=(0, 1, 0), fovx=FOVX, near=1e-2, far=100.0)
    return SceneDesc(vertices, indices, meshes, transforms, np.array([(0, 0), (1, 1)], INSTANCE_DTYPE), [make_material("default"), make_material("grey", diffuse_mul=(200, 200, 200))],
                     [make_light(abi.LIGHT_OMNI, "lamp", position=(0, 0, -1), intensity=5.0)], None, camera, make_meta(centre=(0, 0, -6), radius=15.0))


def focal(cam):
    """pixels per unit of x / z (the pixels are square: (W/2) p0 = (H/2) |p5|)"""
    _, c2s = glaze_amd.host_project_constants(cam, W, H)
    fx, fy = (W / 2.0) * abs(float(c2s[0])), (H / 2.0) * abs(float(c2s[5]))
    assert abs(fx - fy) <= 1e-5 * fx
    return fx, c2s


def world_points(motion_w, fpx):
    """the world point every pixel centre shows in the current state (camera at the origin looking down -z)"""
    py, px = np.mgrid[0:H, 0:W]
    depth = np.where(bits(motion_w) == 1, D1, D2)
    return np.stack([(px + 0.5 - W / 2.0) / fpx * depth, -(py + 0.5 - H / 2.0) / fpx * depth, -depth], -1)


def test_closed_form_camera_translation(instance):
    desc = wall_and_card()
    ren = glaze_amd.RayTraceRenderer.new(instance, make_scene(instance, desc), W, H)
    fpx, c2s = focal(desc.camera)
    # prev eye = (dx, dy, 0): a wall point's previous pixel is its current one + F (-dx, dy) / D2 = + (3.5, 2.5)
    dx, dy = -3.5 * D2 / fpx, 2.5 * D2 / fpx
    prev_cam = make_camera(position=(dx, dy, 0), target=(dx, dy, -100), up=(0, 1, 0), fovx=FOVX, near=1e-2, far=100.0)
    m = ren.read_motion(prev_cam)
    ids = bits(m[..., 3])
    wall, card = ids == 0, ids == 1
    assert wall.sum() + card.sum() == W * H and card.sum() > 300
    P = world_points(m[..., 3], fpx)
    eye = np.array([float(np.float32(dx)), float(np.float32(dy)), 0.0])
    bx, by, bz = projection_bounds(c2s, True, W, H, P.reshape(-1, 3), eye, -P.reshape(-1, 3)[:, 2], None)
    bx, by, bz = bx.reshape(H, W), by.reshape(H, W), bz.reshape(H, W)
    scale = np.where(card, D2 / D1, 1.0)
    ex, ey = np.abs(m[..., 0] - 3.5 * scale), np.abs(m[..., 1] - 2.5 * scale)
    z_want = np.linalg.norm(P - eye, axis=-1)
    ez = np.abs(m[..., 2] - z_want) / z_want
    print("translation: largest error / bound: x %.3f, y %.3f, z' %.3f" % ((ex / bx).max(), (ey / by).max(), (ez / bz).max()))
    assert (ex <= bx).all() and (ey <= by).all() and (ez <= bz).all()
    # reprojection: a smooth previous colour, the previous planes from read_aov in the previous state
    ren.update_camera(prev_cam)
    prev0, prev1 = ren.read_aov(0), ren.read_aov(1)
    ren.update_camera(desc.camera)
    yy, xx = np.mgrid[0:H, 0:W]
    prev_color = np.stack([1.0 + 0.5 * np.sin(xx / 9.0), 0.8 + 0.3 * np.cos(yy / 7.0), 0.2 + xx / 200.0 + yy / 300.0, np.ones((H, W))], -1).astype(np.float32)
    out = ren.reproject(prev_cam, prev_color, prev0, prev1)
    prev_ids = bits(prev1[..., 3])
    qx, qy = xx + m[..., 0].astype(np.float64), yy + m[..., 1].astype(np.float64)
    x0, y0 = np.floor(qx).astype(np.int64), np.floor(qy).astype(np.int64)
    ax, ay = qx - x0, qy - y0
    sw, acc, n_wall = np.zeros((H, W)), np.zeros((H, W, 3)), np.zeros((H, W), np.int64)
    for tdy in (0, 1):
        for tdx in (0, 1):
            tx, ty = x0 + tdx, y0 + tdy
            inside = (tx >= 0) & (tx < W) & (ty >= 0) & (ty < H)
            ix, iy = np.clip(tx, 0, W - 1), np.clip(ty, 0, H - 1)
            is_wall = inside & (prev_ids[iy, ix] == 0)
            wt = (ax if tdx else 1.0 - ax) * (ay if tdy else 1.0 - ay)
            sw += np.where(is_wall, wt, 0.0)
            acc += np.where(is_wall[..., None], wt[..., None] * prev_color[iy, ix, :3].astype(np.float64), 0.0)
            n_wall += is_wall
    full, none, mixed = wall & (n_wall == 4), wall & (n_wall == 0), wall & (n_wall > 0) & (n_wall < 4)
    assert full.sum() > 5000 and none.sum() > 100 and mixed.sum() > 50, (full.sum(), none.sum(), mixed.sum())
    assert (bits(out[none]) == 0).all()                                               # disoccluded: every tap was card (or outside the frame)
    some = full | mixed
    want = acc[some] / sw[some][:, None]
    assert (np.abs(out[some][:, :3] - want) <= 1e-5 * np.abs(want)).all()
    assert (np.abs(out[some][:, 3] - sw[some]) <= 1e-5).all() and (np.abs(out[full][:, 3] - 1.0) <= 1e-5).all()


def test_closed_form_card_rotation(instance):
    desc = wall_and_card()
    ren = glaze_amd.RayTraceRenderer.new(instance, make_scene(instance, desc), W, H)
    fpx, c2s = focal(desc.camera)
    theta = 0.3
    c, s = np.cos(theta), np.sin(theta)
    back = np.eye(4)
    back[:2, :2] = [[c, s], [-s, c]]                                                  # the card's previous state: turned by -theta about z
    prev_xf = np.stack([np.eye(4).T.reshape(16), back.T.reshape(16)]).astype(np.float32)
    m = ren.read_motion(desc.camera, prev_xf)
    ids = bits(m[..., 3])
    wall, card = ids == 0, ids == 1
    assert card.sum() > 300
    P = world_points(m[..., 3], fpx).reshape(-1, 3)
    bx, by, _ = projection_bounds(c2s, True, W, H, P, (0, 0, 0), -P[:, 2], None)
    bx, by = bx.reshape(H, W), by.reshape(H, W)
    # a screen vector is F (X, -Y) / D, y down: turning the world by -theta about z turns it by [[c, -s], [s, c]] about the image centre
    py, px = np.mgrid[0:H, 0:W]
    sx, sy = px + 0.5 - W / 2.0, py + 0.5 - H / 2.0
    want_x, want_y = np.where(card, (c * sx - s * sy) - sx, 0.0), np.where(card, (s * sx + c * sy) - sy, 0.0)
    ex, ey = np.abs(m[..., 0] - want_x), np.abs(m[..., 1] - want_y)
    print("rotation: largest error / bound: x %.3f, y %.3f; wall motion %.3g px" % ((ex / bx).max(), (ey / by).max(), np.abs(m[wall][:, :2]).max()))
    assert (ex <= bx).all() and (ey <= by).all()
    assert (np.abs(m[card][:, 2] - np.linalg.norm(P.reshape(H, W, 3)[card], axis=-1)) <= 1e-5 * D1).all()


# ---------------------------------------------------------------------------------------------------------------------
# 7. device == host, bit for bit
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cameras()))
def test_device_projection_equals_host_projection(instance, name):
    cam = cameras()[name]
    pts = projection_points(cam, 4096, seed=11)
    for w, h in ((128, 72), (1920, 1080)):
        host, dev = glaze_amd.host_project_points(cam, w, h, pts), instance.debug_project_points(cam, w, h, pts)
        differ = (bits(host) != bits(dev)).any(-1)
        assert not differ.any(), "%d points differ, first %s" % (differ.sum(), pts[differ][0])


@pytest.mark.parametrize("size,shift", REPROJECT_CASES + [((1, 1), (0.25, -0.25)), ((97, 61), (-6.5, 3.25)), ((1920, 1080), (11.75, -4.5))])
def test_device_reprojection_equals_host_reprojection(instance, size, shift):
    motion, color, aov0, aov1 = reproject_inputs(size[0], size[1], seed=size[0] + int(4 * shift[0]), shift=shift)
    for params in ({}, dict(depth_tolerance=0.004), dict(depth_tolerance=0.5)):
        host = glaze_amd.host_reproject(motion, color, aov0, aov1, **params)
        dev = instance.debug_reproject(motion, color, aov0, aov1, **params)
        differ = (bits(host) != bits(dev)).any(-1)
        assert not differ.any(), "%d pixels differ (%s), first at %s" % (differ.sum(), params, np.argwhere(differ)[0])
    if size != (1, 1):
        assert (host[..., 3] > 0).mean() > 0.3
    with pytest.raises(glaze_amd.GlazeError) as e:
        instance.debug_reproject(motion, color, aov0, aov1, depth_tolerance=0.0)
    assert e.value.status == -4


# ---------------------------------------------------------------------------------------------------------------------
# 8. end to end
# ---------------------------------------------------------------------------------------------------------------------
def previous_planes(ren, desc, prev_cam, prev_xf):
    """read_aov of the previous state, then back to the current one"""
    ren.update_camera(prev_cam)
    ren.update_transforms(prev_xf)
    planes = ren.read_aov(0), ren.read_aov(1)
    ren.update_camera(desc.camera)
    ren.update_transforms(desc.transforms)
    return planes


def test_reproject_is_the_host_rule_on_the_motion_plane(instance):
    desc = forest_scene(40)
    ren = glaze_amd.RayTraceRenderer.new(instance, make_scene(instance, desc, "two_level"), W, H)
    prev_cam, prev_xf = moved_camera(desc.camera), moved_transforms(desc.transforms, seed=4, every=3)
    prev0, prev1 = previous_planes(ren, desc, prev_cam, prev_xf)
    prev_color = synthetic_frame(W, H, seed=8)[0]
    motion = ren.read_motion(prev_cam, prev_xf)
    for params in ({}, dict(depth_tolerance=0.1)):
        out = ren.reproject(prev_cam, prev_color, prev0, prev1, prev_xf, **params)
        assert np.array_equal(bits(out), bits(glaze_amd.host_reproject(motion, prev_color, prev0, prev1, **params))), params
    hits = np.isfinite(motion[..., 2])
    print("moved forest: %.1f %% of %d hit pixels receive history" % (100.0 * (out[..., 3] > 0)[hits].mean(), hits.sum()))
    assert (out[..., 3] > 0)[hits].mean() > 0.5


def test_motion_does_not_depend_on_the_guide_mode(instance):
    desc = mirror_room_scene(mirror=True)
    ren = glaze_amd.RayTraceRenderer.new(instance, make_scene(instance, desc), W, H)
    prev_cam, prev_xf = moved_camera(desc.camera, shift=(0.2, 0.05, -0.1), turn=(0.3, 0.0, 0.0)), moved_transforms(desc.transforms, seed=6)
    first = ren.read_motion(prev_cam, prev_xf)
    aov = ren.read_aov(1)
    ren.set_guide_mode("through_specular", 4)
    assert not np.array_equal(bits(ren.read_aov(1)), bits(aov))                       # the chain does run here
    assert np.array_equal(bits(ren.read_motion(prev_cam, prev_xf)), bits(first))
    assert np.array_equal(bits(first[..., 3]), bits(aov[..., 3]))                     # segment 0's instances


# ---------------------------------------------------------------------------------------------------------------------
# 9. it disturbs nothing
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("config", ["two_kernels", "path", "chains3"])
def test_motion_and_reprojection_do_not_disturb_the_accumulation(instance, config):
    desc = atrium_scene(sponza_like=True, texture_size=64, sky_size=(64, 32))
    prev_cam = moved_camera(desc.camera, shift=(0.2, 0.05, -0.1), turn=(0.3, 0.0, 0.0))
    prev_xf = moved_transforms(desc.transforms, seed=2)
    frame = synthetic_frame(150, 83, seed=3)

    def renderer():
        r = glaze_amd.RayTraceRenderer.new(instance, glaze_amd.RayTraceScene.from_desc(instance, desc), 150, 83)
        r.set_seed(21)
        r.set_depth(4)
        if config == "chains3":
            r.set_chains(3)
        else:
            r.set_launch_mode(config)
        return r

    a, b = renderer(), renderer()
    a.step(24)
    b.step(7)
    b.read_motion(prev_cam, prev_xf)
    b.read_motion(prev_cam)
    b.reproject(prev_cam, frame[0], frame[1], frame[2], prev_xf)
    b.step(17)
    assert np.array_equal(bits(a.read_hdr()), bits(b.read_hdr()))
    assert np.array_equal(bits(a.read_result()), bits(b.read_result()))
    assert a.stats().launches == b.stats().launches == 24
    for which in (0, 1):
        assert np.array_equal(bits(a.read_aov(which)), bits(b.read_aov(which)))
    assert np.array_equal(bits(a.read_denoised()), bits(b.read_denoised()))


# ---------------------------------------------------------------------------------------------------------------------
# 10. ABI arguments
# ---------------------------------------------------------------------------------------------------------------------
def test_motion_abi_arguments(instance):
    desc = forest_scene(40)
    ren = glaze_amd.RayTraceRenderer.new(instance, make_scene(instance, desc, "two_level"), W, H)
    ren.set_seed(5)
    ren.step(3)
    prev_cam = moved_camera(desc.camera)
    good = ren.read_motion(prev_cam, desc.transforms)
    hdr = ren.read_hdr()
    frame = synthetic_frame(W, H, seed=3)
    lib = abi.lib()
    out = np.full((H, W, 4), 7.0, np.float32)
    cam_p, out_p = C.cast(C.byref(prev_cam), C.c_void_p), out.ctypes.data_as(C.c_void_p)
    planes = [f.ctypes.data_as(C.c_void_p) for f in frame[:3]]
    xf = np.ascontiguousarray(desc.transforms[:-1])
    calls = [lambda: lib.glz_renderer_read_motion(ren._h, cam_p, xf.ctypes.data_as(C.c_void_p), xf.shape[0], out_p),       # wrong count
             lambda: lib.glz_renderer_read_motion(ren._h, None, None, 0, out_p),
             lambda: lib.glz_renderer_read_motion(ren._h, cam_p, None, 0, None),
             lambda: lib.glz_renderer_reproject(ren._h, cam_p, xf.ctypes.data_as(C.c_void_p), xf.shape[0], planes[0], planes[1], planes[2], None, out_p),
             lambda: lib.glz_renderer_reproject(ren._h, None, None, 0, planes[0], planes[1], planes[2], None, out_p),
             lambda: lib.glz_renderer_reproject(ren._h, cam_p, None, 0, planes[0], planes[1], planes[2], None, None),
             lambda: lib.glz_renderer_reproject(ren._h, cam_p, None, 0, None, planes[1], planes[2], None, out_p)]
    for i, call in enumerate(calls):
        assert call() == -4, i
    for bad in (0.0, -1.0, np.nan, np.inf):
        with pytest.raises(glaze_amd.GlazeError) as e:
            ren.reproject(prev_cam, frame[0], frame[1], frame[2], depth_tolerance=bad)
        assert e.value.status == -4
    assert (out == 7.0).all()                                                          # nothing was written
    assert np.array_equal(bits(ren.read_hdr()), bits(hdr)) and ren.stats().launches == 3
    assert np.array_equal(bits(ren.read_motion(prev_cam)), bits(good))                 # NULL transforms: the count is ignored
    ren.set_partition(0, 2)
    assert np.array_equal(bits(ren.read_motion(prev_cam, desc.transforms)), bits(good))
    assert ren.reproject(prev_cam, frame[0], frame[1], frame[2]).shape == (H, W, 4)
