"""The result image and the launch count are made when the images are read (k_finalize, Renderer::settle), not in every launch: a launch
leaves only -(its ordinal) in cumulative.w of the pixels that call update_result, and a pixel that does not update touches nothing.
Whatever is read -- hdr, result, the device exports, the exchange of set_devices -- has to be what the eager update_count /
update_result of the oracle holds, bit for bit: after launches in which pixels skip updates (specular bounces, misses without a sky)
or never update at all, across changes of the exposure with no read in between, in every launch shape, and when the first thing that
looks is a device export.

Frames are 60 x 45 (one tile) and 150 x 83 (3 x 2 tiles), both with edge tiles that reach past the image; depth 4; at most 20 launches
a case.  The oracle's images of a sequence are computed once per (scene, frame, integrator) and shared.
"""
import numpy as np
import pytest

import glaze_amd
from glaze_amd import abi
from glaze_amd.scene_desc import INSTANCE_DTYPE, MESH_DTYPE, make_camera, make_light, make_material
from glaze_amd.scenes import cube_scene
from oracle.pyoracle import OracleRenderer, OracleScene

from helpers import DeviceArray

pytestmark = pytest.mark.gpu

FRAMES = [(60, 45), (150, 83)]
DEPTH = 4
SEED = 5
SEQUENCE = ((1.0, 2), (0.5, 3), (2.0, 1))      # (exposure, launches): two changes with launches between them, nothing read in between
LAUNCHES = sum(n for _, n in SEQUENCE)


def bits(a):
    return np.nan_to_num(a, nan=-1.0).view(np.uint32)


def open_cube(sky):
    """The cube from inside with its +z wall taken out, the +x wall a mirror and the ceiling glass, under a sun that shines in through the
    opening; the camera looks down at the edge between the opening and the mirror, over the diffuse floor.  Without a sky the camera rays
    that leave never update their pixel, the mirror's and the glass's pixels skip the launches of their specular bounces, and paths that
    leave behind a diffuse bounce only count.  With the sky every miss at bounce 0 (or behind a specular bounce) updates."""
    desc = cube_scene(material_type=abi.MAT_LAMBERT)
    desc.materials.append(make_material("mirror", mtype=abi.MAT_MIRROR))
    desc.materials.append(make_material("glass", mtype=abi.MAT_GLASS, ior=1.5))
    # cube_scene's faces in order: +y, +z, -x, -y, +x, -z, six indices each
    faces = [(0, 4), (2, 2), (3, 2), (4, 3), (5, 2)]                      # (face, material): +z is left out
    desc.meshes = np.array([(i, m, 6 * f, 6) for i, (f, m) in enumerate(faces)], MESH_DTYPE)
    desc.instances = np.array([(i, 0) for i in range(len(faces))], INSTANCE_DTYPE)
    desc.lights = [make_light(abi.LIGHT_SUN, "sun", direction=(-0.25, -0.45, -0.85), intensity=1.5)]
    if sky:
        desc.lights.append(make_light(abi.LIGHT_SKY, "sky", resource_id=1, intensity=0.3, yaw=20, pitch=75, roll=10))
    desc.camera = make_camera(position=(-0.2, 0.1, -0.3), target=(60, -70, 100), up=(0, 1, 0), fovx=np.float32(np.radians(np.float32(80.0))),
                              near=1e-3, far=100.0)
    return desc


def new_pair(instance, desc, w, h, integrator=glaze_amd.Integrator.PATH_TRACE):
    r = glaze_amd.RayTraceRenderer.new(instance, glaze_amd.RayTraceScene.from_desc(instance, desc), w, h)
    o = OracleRenderer(OracleScene(desc), w, h)
    for x in (r, o):
        x.set_depth(DEPTH)
        x.set_seed(SEED)
    r.set_integrator(integrator)
    o.set_integrator(integrator.value)
    return r, o


def new_renderer(instance, desc, w, h):
    r = glaze_amd.RayTraceRenderer.new(instance, glaze_amd.RayTraceScene.from_desc(instance, desc), w, h)
    r.set_depth(DEPTH)
    r.set_seed(SEED)
    return r


def run_sequence(x):
    for exposure, n in SEQUENCE:
        x.set_exposure(exposure)
        x.step(n)


_sky_reference = {}


def sky_reference(w, h, integrator=glaze_amd.Integrator.PATH_TRACE):
    """(hdr, result) of the oracle after SEQUENCE on the cube with the sky; computed once, handed out read-only"""
    key = (w, h, integrator)
    if key not in _sky_reference:
        o = OracleRenderer(OracleScene(open_cube(True)), w, h)
        o.set_integrator(integrator.value)
        o.set_depth(DEPTH)
        o.set_seed(SEED)
        run_sequence(o)
        hdr, res = o.read_hdr(), o.read_result()
        hdr.setflags(write=False)
        res.setflags(write=False)
        _sky_reference[key] = (hdr, res)
    return _sky_reference[key]


def assert_images(r, hdr, res, launches, tag=""):
    g, gr = r.read_hdr(), r.read_result()
    assert (g[..., 3] == float(launches)).all(), tag + ": every pixel of the image has counted every launch"
    assert np.array_equal(bits(g), bits(hdr)), "%s: hdr differs in %d pixels" % (tag, int((bits(g) != bits(hdr)).any(-1).sum()))
    assert np.array_equal(bits(gr), bits(res)), "%s: result differs in %d pixels" % (tag, int((bits(gr) != bits(res)).any(-1).sum()))
    assert not gr[~res.any(-1)].any(), tag + ": a pixel that never updated has a result"
    return g, gr


@pytest.mark.parametrize("w,h", FRAMES)
def test_specular_pixels_and_pixels_that_never_update(instance, w, h):
    r, o = new_pair(instance, open_cube(False), w, h)
    r.step(1)
    o.step(1)
    hdr, res = o.read_hdr(), o.read_result()
    never = ~res.any(-1)
    assert never.any() and (~never).any()                       # camera rays that leave through the opening; lit walls
    assert_images(r, hdr, res, 1, "one launch")
    r.step(3)
    o.step(3)
    hdr, res = o.read_hdr(), o.read_result()
    never = ~res.any(-1)
    assert never.any()
    # some pixel updated in an earlier launch and not in the last one (a specular bounce, a miss behind a diffuse one): its result keeps the divisor of its own launch
    lit = ~never
    assert (bits(res[..., :3][lit]) != bits((hdr[..., :3] * np.float32(1.0) / hdr[..., 3:4])[lit])).any()
    g, gr = assert_images(r, hdr, res, 4, "four launches")
    g2, gr2 = r.read_hdr(), r.read_result()                     # nothing launched in between: the resolve changes nothing the second time
    assert np.array_equal(bits(g2), bits(g)) and np.array_equal(bits(gr2), bits(gr))
    assert_images(r, hdr, res, 4, "read again")


@pytest.mark.parametrize("w,h", FRAMES)
def test_exposure_changes_without_a_read_in_between(instance, w, h):
    r, o = new_pair(instance, open_cube(False), w, h)
    for x in (r, o):
        x.set_exposure(0.7)                                      # before the first launch
        x.step(2)
        x.set_exposure(0.7)                                      # the value already set: nothing to resolve
        x.step(1)
        x.set_exposure(1.0)
        run_sequence(x)                                          # 1.0 again, then two real changes with launches between them
    assert_images(r, o.read_hdr(), o.read_result(), 3 + LAUNCHES, "exposure sequence")
    for x in (r, o):
        x.restart()
        x.set_exposure(1.5)                                      # directly after a restart: the abandoned frame has nothing to resolve
        x.step(2)
    assert_images(r, o.read_hdr(), o.read_result(), 2, "after a restart")
    for x in (r, o):
        x.set_exposure(0.25)                                     # a change, then a read with no launch after it: the resolved result stays
    assert_images(r, o.read_hdr(), o.read_result(), 2, "a change with nothing launched after it")


def _two_kernels(r):
    r.set_launch_mode("two_kernels")


def _per_wave(r):
    r.set_launch_mode("path")


def _three_chains(r):
    r.set_launch_mode("two_kernels")
    r.set_chains(3)


@pytest.mark.parametrize("w,h", FRAMES)
@pytest.mark.parametrize("shape", [_two_kernels, _per_wave, _three_chains], ids=["two_kernels", "per_wave", "three_chains"])
def test_launch_shapes_with_a_sky(instance, w, h, shape):
    hdr, res = sky_reference(w, h)
    r = new_renderer(instance, open_cube(True), w, h)
    shape(r)
    run_sequence(r)
    assert_images(r, hdr, res, LAUNCHES, shape.__name__)


@pytest.mark.parametrize("w,h", FRAMES)
def test_direct_light_integrator_with_a_sky(instance, w, h):
    hdr, res = sky_reference(w, h, glaze_amd.Integrator.DIRECT)
    r = new_renderer(instance, open_cube(True), w, h)
    r.set_integrator(glaze_amd.Integrator.DIRECT)
    run_sequence(r)
    assert_images(r, hdr, res, LAUNCHES, "direct")


@pytest.mark.parametrize("w,h", FRAMES)
def test_one_rank_of_a_partition_with_a_sky(instance, w, h):
    hdr, res = sky_reference(w, h)
    owner = np.zeros((h, w), np.uint16)
    abi.check(abi.lib().glz_host_tile_owner(w, h, 3, owner.ctypes.data))
    mine = owner == 1
    r = new_renderer(instance, open_cube(True), w, h)
    r.set_partition(1, 3)
    run_sequence(r)
    g, gr = r.read_hdr(), r.read_result()
    assert not g[~mine].any() and not gr[~mine].any()
    assert mine.any() == bool(g.any())                           # (the one-tile frame belongs to rank 0: nothing here)
    assert (g[..., 3][mine] == float(LAUNCHES)).all()
    assert np.array_equal(bits(g[mine]), bits(hdr[mine])) and np.array_equal(bits(gr[mine]), bits(res[mine]))


@pytest.mark.parametrize("w,h", FRAMES)
def test_device_exports_are_the_first_to_look(instance, w, h):
    hdr, res = sky_reference(w, h)
    r = new_renderer(instance, open_cube(True), w, h)
    run_sequence(r)
    frame = DeviceArray((h, w, 4))
    r.export_device(1, frame.ptr)                                # nothing has been read before
    assert np.array_equal(bits(frame.numpy()), bits(res))
    r.export_device(0, frame.ptr)
    assert np.array_equal(bits(frame.numpy()), bits(hdr))
    p = new_renderer(instance, open_cube(True), w, h)
    p.set_launch_mode("two_kernels")
    p.set_chains(2)                                              # (one tile: one chain)
    run_sequence(p)
    packed = DeviceArray((p.packed_pixels(0, 1), 4))
    p.export_packed(1, packed.ptr)                               # nothing has been read before
    frame.upload(np.zeros((h, w, 4), np.float32))
    p.scatter_packed(0, 1, packed.ptr, frame.ptr)
    assert np.array_equal(bits(frame.numpy()), bits(res))
    p.export_packed(0, packed.ptr)
    p.scatter_packed(0, 1, packed.ptr, frame.ptr)
    assert np.array_equal(bits(frame.numpy()), bits(hdr))


@pytest.mark.parametrize("w,h", FRAMES)
def test_two_loopback_devices_after_an_exposure_change(instance, monkeypatch, w, h):
    monkeypatch.setenv("GLAZE_MULTI_LOOPBACK", "1")
    hdr, res = sky_reference(w, h)
    one = new_renderer(instance, open_cube(True), w, h)
    run_sequence(one)
    hdr1, res1 = assert_images(one, hdr, res, LAUNCHES, "one device")
    r = new_renderer(instance, open_cube(True), w, h)
    r.set_devices([instance.device] * 2)
    run_sequence(r)
    g, gr = r.read_hdr(), r.read_result()
    assert np.array_equal(bits(g), bits(hdr1)) and np.array_equal(bits(gr), bits(res1))
