"""First-hit feature buffers (glz_renderer_read_aov) and the edge-aware denoiser (glz_renderer_read_denoised) on the device.

The device filter must equal the host filter bit for bit (the host filter is checked against a float64 restatement of the
specification in tests/test_denoise_host.py); the first-hit pass must equal the oracle's closest hits of the same centre rays bit
for bit; neither may disturb a running accumulation.
"""
import os
import subprocess

import numpy as np
import pytest
from PIL import Image

import glaze_amd
from glaze_amd import abi
from glaze_amd.scene_desc import _clone
from glaze_amd.scenes import atrium_scene, cube_scene, forest_scene, mirror_room_scene
from oracle.pyoracle import OracleScene

from conftest import MATTEST
from denoise_ref import synthetic_frame
from helpers import camera_rays, desc_from_oracle_parse

pytestmark = pytest.mark.gpu

CLI = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "glaze_amd", "csrc", "glaze-cli")
BSDF_LAMBERT, BSDF_UBER = 4, 14          # RTMaterial::bsdf_index (device/types.h)
NON_DEFAULT = (dict(sigma_color=1.5, sigma_depth=0.25, normal_power_log2=3, eps_albedo=0.05, eps_depth=1e-2, eps_color=1e-4),
               dict(sigma_color=16.0, sigma_depth=8.0, normal_power_log2=0, eps_albedo=1e-6, eps_depth=0.0, eps_color=1e-12))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------------
# 4. device filter == host filter, bit for bit
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(150, 83), (97, 61), (1920, 1080)])
def test_device_filter_equals_host_filter(instance, size):
    result, aov0, aov1, _ = synthetic_frame(size[0], size[1], seed=size[0] + 1)
    result[size[1] // 2, size[0] // 3, 0] = np.nan                  # non-finite pixels take the same way on both sides
    result[size[1] // 2 + 5, size[0] // 3, 2] = np.inf
    for iterations in (1, 2, 3, 4, 5):
        for params in ({},) + NON_DEFAULT:
            host = glaze_amd.host_denoise(result, aov0, aov1, iterations=iterations, **params)
            dev = instance.debug_denoise(result, aov0, aov1, iterations=iterations, **params)
            differ = (bits(host) != bits(dev)).any(-1)
            assert not differ.any(), "%d pixels differ (iterations %d, %s), first at %s" % (
                differ.sum(), iterations, params, np.argwhere(differ)[0])
    with pytest.raises(glaze_amd.GlazeError) as e:
        instance.debug_denoise(result, aov0, aov1, iterations=9)
    assert e.value.status == -4


# ---------------------------------------------------------------------------------------------------------------------
# 5. first-hit pass == oracle
# ---------------------------------------------------------------------------------------------------------------------
def small_atrium():
    return atrium_scene(sponza_like=True, texture_size=64, sky_size=(64, 32))


def first_hit_scenes():
    return {"cube": (cube_scene, "auto"), "mattest": (lambda: desc_from_oracle_parse(MATTEST), "auto"),
            "forest": (lambda: forest_scene(40), "two_level"), "atrium": (small_atrium, "auto")}


def restate_first_hit(desc, orc, o, d, t, tri, inst, u, v):
    """albedo (float32, the kernel's operation order) and normal (float64) of the hits the oracle reports; which hits have no normal map,
    which have one, which lie on alpha-tested geometry"""
    n = t.shape[0]
    hit = np.isfinite(t)
    meshes = {int(m["id"]): m for m in desc.meshes}
    inst_mesh = [meshes[int(i["mesh_id"])] for i in desc.instances]
    base = np.concatenate([[0], np.cumsum([int(m["index_count"]) // 3 for m in inst_mesh])]).astype(np.int64)
    ii = np.where(hit, inst, 0).astype(np.int64)
    assert (inst[hit] < len(inst_mesh)).all()
    local = np.where(hit, tri.astype(np.int64) - base[ii], 0)
    counts = np.array([int(m["index_count"]) // 3 for m in inst_mesh], np.int64)
    assert (local >= 0).all() and (local[hit] < counts[ii][hit]).all()
    first = np.array([int(m["index_offset"]) for m in inst_mesh], np.int64)[ii] + 3 * local
    vid = np.stack([desc.indices[first + k] for k in range(3)], -1)
    mat_id = np.array([int(m["material"]) for m in inst_mesh], np.int64)[ii]
    xf_id = np.array([int(i["transform_id"]) for i in desc.instances], np.int64)[ii]
    vt, vn = desc.vertices["vt"][vid], desc.vertices["vn"][vid]             # n x 3 x 2, n x 3 x 3
    f = np.float32
    b1, b2 = u.astype(f), v.astype(f)
    b0 = (f(1.0) - b1) - b2
    uv = np.stack([(vt[:, 0, k] * b0 + vt[:, 1, k] * b1) + vt[:, 2, k] * b2 for k in range(2)], -1).astype(f)
    raw = orc.rt_materials().reshape(-1, 208)
    bsdf = raw[:, 180:184].copy().view(np.uint32)[:, 0]
    diffuse = raw[:, 160:164].copy().view(np.uint32)[:, 0]
    normal_tex = raw[:, 176:180].copy().view(np.uint32)[:, 0]
    mul = raw[:, 0:12].copy().view(np.float32)
    albedo = np.ones((n, 3), f)
    for m in np.unique(mat_id[hit]):
        if bsdf[m] not in (BSDF_LAMBERT, BSDF_UBER):
            continue
        sel = hit & (mat_id == m)
        albedo[sel] = (orc.sample_texture(int(diffuse[m]), uv[sel])[:, :3] * mul[m][None, :]).astype(f)
    # normal: barycentric vertex normals, (normal map in the triangle's frame,) inverse-transpose, normalise, face the camera -- float64
    ns = (vn[:, 0].astype(np.float64) * b0[:, None] + vn[:, 1] * b1[:, None].astype(np.float64)) + vn[:, 2] * b2[:, None].astype(np.float64)
    deriv = orc.derivatives().astype(np.float64)[first // 3]                                      # per object-space triangle: normal, dpdu, dpdv (3 x vec4)
    ng, dpdu = deriv[:, 0:3], deriv[:, 4:7]
    mapped = hit & (normal_tex[mat_id] != 0)
    with np.errstate(all="ignore"):
        for m in np.unique(mat_id[mapped]):
            sel = mapped & (mat_id == m)
            vmap = orc.sample_texture(int(normal_tex[m]), uv[sel])[:, :3].astype(np.float64) * 2.0 - 1.0
            s_ = dpdu[sel] / np.linalg.norm(dpdu[sel], axis=-1, keepdims=True)
            n_ = ns[sel]                                                                          # the frame's normal is NOT normalised
            t_ = np.cross(n_, s_)
            t_ /= np.linalg.norm(t_, axis=-1, keepdims=True)
            wv = s_ * vmap[:, 0:1] + t_ * vmap[:, 1:2] + n_ * vmap[:, 2:3]
            wv /= np.linalg.norm(wv, axis=-1, keepdims=True)
            ns[sel] = wv * np.sign((ng[sel] * wv).sum(-1, keepdims=True))
        M = desc.transforms.reshape(-1, 4, 4).transpose(0, 2, 1).astype(np.float64)[:, :3, :3]    # column-major -> row-major 3 x 3
        inv_t = np.linalg.inv(M).transpose(0, 2, 1)
        nw = np.einsum("nij,nj->ni", inv_t[xf_id], ns)
        nw /= np.linalg.norm(nw, axis=-1, keepdims=True)
        nw = np.where((nw * d.astype(np.float64)).sum(-1, keepdims=True) > 0, -nw, nw)
    plain = hit & (normal_tex[mat_id] == 0)
    alpha_tested = hit & (raw[:, 172:176].copy().view(np.uint32)[:, 0][mat_id] != 0)
    return albedo, nw, plain, mapped, alpha_tested


@pytest.mark.parametrize("size", [(256, 144), (150, 83)])
@pytest.mark.parametrize("name", ["cube", "mattest", "forest", "atrium"])
def test_first_hit_pass_equals_the_oracle(instance, name, size):
    make, levels = first_hit_scenes()[name]
    desc = make()
    w, h = size
    instance.set_as_levels(levels)
    try:
        scene = glaze_amd.RayTraceScene.from_desc(instance, desc)
    finally:
        instance.set_as_levels("auto")
    if levels == "two_level":
        assert scene.info().as_levels == 2
    ren = glaze_amd.RayTraceRenderer.new(instance, scene, w, h)
    o, d = ren.debug_camera_rays((0.5, 0.5))
    ho, hd = camera_rays(ren.push_constants(), w, h)
    assert desc.camera.type == abi.CAMERA_PERSPECTIVE
    assert np.abs(o.reshape(-1, 3) - ho).max() <= 1e-6 * max(1.0, np.abs(ho).max()) and np.abs(d.reshape(-1, 3) - hd).max() <= 1e-6
    orc = OracleScene(desc)
    t, tri, inst, u, v = orc.trace_closest(o.reshape(-1, 3), d.reshape(-1, 3), tmin=1e-4)
    hit = np.isfinite(t)
    assert hit.any()
    nd = ren.read_aov("normal_depth").reshape(-1, 4)
    ai = ren.read_aov("albedo_instance").reshape(-1, 4)
    assert np.array_equal(bits(nd[:, 3]), bits(np.where(hit, t, np.float32(np.inf))))
    assert np.array_equal(bits(ai[:, 3]), np.where(hit, inst, np.uint32(0xFFFFFFFF)).astype(np.uint32))
    albedo, normal, plain, mapped, alpha_tested = restate_first_hit(desc, orc, o.reshape(-1, 3), d.reshape(-1, 3), t, tri, inst, u, v)
    if name == "atrium":                                                       # what this scene is here for
        assert mapped.sum() > 1000 and alpha_tested.sum() > 100, (mapped.sum(), alpha_tested.sum())
    differ = (bits(ai[:, :3]) != bits(albedo)).any(-1)
    assert not differ.any(), "%d albedo values differ, first at %s" % (differ.sum(), np.argwhere(differ)[0])
    assert (nd[~hit, :3] == 0).all()
    err = np.abs(nd[plain, :3].astype(np.float64) - normal[plain])
    print("%s %dx%d: %d hits, normal max abs err %.3g" % (name, w, h, hit.sum(), err.max() if err.size else 0.0))
    assert err.size == 0 or err.max() <= 1e-5
    # Normal-mapped hits (the issue sets no bound for them): the same restatement with the map applied in the triangle's frame.  About
    # twice the rounded operations of the plain case (two more normalisations, a cross product, the frame product): twice its bound.
    err = np.abs(nd[mapped, :3].astype(np.float64) - normal[mapped])
    if err.size:
        print("  %d normal-mapped hits, normal max abs err %.3g; %d hits on alpha-tested geometry" % (mapped.sum(), err.max(), alpha_tested.sum()))
        assert err.max() <= 2e-5
    if name == "mattest":
        # the oracle needs a scene description, which its own reader made; the library's reader (parse) must lead to the same planes
        parsed = glaze_amd.RayTraceRenderer.new(instance, glaze_amd.RayTraceScene.new(instance, glaze_amd.parse(MATTEST)), w, h)
        assert np.array_equal(bits(parsed.read_aov(0)), bits(nd.reshape(h, w, 4))) and np.array_equal(bits(parsed.read_aov(1)), bits(ai.reshape(h, w, 4)))
    length = np.linalg.norm(nd[hit, :3].astype(np.float64), axis=-1)
    assert np.abs(length - 1.0).max() <= 1e-5
    assert ((nd[hit, :3].astype(np.float64) * d.reshape(-1, 3)[hit]).sum(-1) <= 0).all()


def test_first_hit_pass_does_not_depend_on_the_render_state(instance, monkeypatch):
    monkeypatch.setenv("GLAZE_MULTI_LOOPBACK", "1")
    desc = small_atrium()
    w, h = 150, 83

    def planes(r):
        return bits(r.read_aov(0)), bits(r.read_aov(1))

    ren = glaze_amd.RayTraceRenderer.new(instance, glaze_amd.RayTraceScene.from_desc(instance, desc), w, h)
    want = planes(ren)
    ren.step(5)
    for got, ref in zip(planes(ren), want):
        assert np.array_equal(got, ref)
    for mode in ("two_kernels", "path"):
        r = glaze_amd.RayTraceRenderer.new(instance, glaze_amd.RayTraceScene.from_desc(instance, desc), w, h)
        r.set_launch_mode(mode)
        r.step(3)
        for got, ref in zip(planes(r), want):
            assert np.array_equal(got, ref), mode
    r = glaze_amd.RayTraceRenderer.new(instance, glaze_amd.RayTraceScene.from_desc(instance, desc), w, h)
    r.set_chains(3)
    r.step(2)
    for got, ref in zip(planes(r), want):
        assert np.array_equal(got, ref)
    r = glaze_amd.RayTraceRenderer.new(instance, glaze_amd.RayTraceScene.from_desc(instance, desc), w, h)
    r.set_devices([instance.device] * 3)
    r.step(2)
    for got, ref in zip(planes(r), want):
        assert np.array_equal(got, ref)
    den = r.read_denoised()                                                # the filter runs on device 0 after the exchange
    assert np.array_equal(bits(den), bits(glaze_amd.host_denoise(r.read_result(), r.read_aov(0), r.read_aov(1))))
    r = glaze_amd.RayTraceRenderer.new(instance, glaze_amd.RayTraceScene.from_desc(instance, desc), w, h)
    r.set_partition(1, 4)
    for got, ref in zip(planes(r), want):
        assert np.array_equal(got, ref)
    # a renderer without a scene: all-miss planes
    empty = glaze_amd.RayTraceRenderer.new(instance, None, 70, 40)
    nd, ai = empty.read_aov(0), empty.read_aov(1)
    assert np.isposinf(nd[..., 3]).all() and (nd[..., :3] == 0).all() and (ai[..., :3] == 1).all()
    assert (bits(ai[..., 3]) == 0xFFFFFFFF).all()


def test_post_buffers_follow_scene_resolution_guide_mode_and_devices(instance, monkeypatch):
    """The lifetime of the post stage's buffers: ONE renderer driven through new scenes, resolutions, guide modes and device counts must
    read, in every state, the bits a fresh renderer created directly in that state reads."""
    monkeypatch.setenv("GLAZE_MULTI_LOOPBACK", "1")
    descs = {"cube": cube_scene(), "room": mirror_room_scene(), "atrium": small_atrium()}

    def scene(name):                                                            # a renderer takes its scene over: one per use
        return glaze_amd.RayTraceScene.from_desc(instance, descs[name])

    # the traversal spill of the first-hit pass is sized by the scene (stack_overflow_depth: 3 * depth + 2 against the 17 entries kept in
    # LDS), not only by the frame: the cube needs the minimum, the atrium more
    assert scene("cube").info().bvh_depth <= 5 and scene("atrium").info().bvh_depth >= 6

    def sideways(cam):
        c = _clone(cam)
        c.position[:] = [a + b for a, b in zip(cam.position[:], (0.3, 0.0, 0.0))]
        c.target[:] = [a + b for a, b in zip(cam.target[:], (0.3, 0.0, 0.0))]
        return c

    reads = {"aov0": lambda r, desc: (r.read_aov(0),), "aov1": lambda r, desc: (r.read_aov(1),),
             "denoised": lambda r, desc: (r.read_denoised(),), "despeckled": lambda r, desc: (r.read_despeckled(),),
             "motion": lambda r, desc: (r.read_motion(sideways(desc.camera)),), "chain": lambda r, desc: r.debug_guide_chain(1)}

    def fresh(name, w, h, guide):
        r = glaze_amd.RayTraceRenderer.new(instance, scene(name), w, h)
        r.set_guide_mode(*guide)
        return r

    def check(state, ren, ref, name, names):
        for r in (ren, ref):
            r.set_seed(17)
            r.set_depth(3)
            r.step(2)
        for read in names:
            got, want = reads[read](ren, descs[name]), reads[read](ref, descs[name])
            assert len(got) == len(want)
            for a, b in zip(got, want):
                assert a.shape == b.shape and np.array_equal(bits(a), bits(b)), (state, read)

    first_hit, through = ("first_hit",), ("through_specular", 2)
    planes = ("aov0", "aov1")
    ren = glaze_amd.RayTraceRenderer.new(instance, scene("cube"), 70, 40)
    check(1, ren, fresh("cube", 70, 40, first_hit), "cube", planes)
    ren.set_guide_mode(*through)
    ren.change_scene(scene("room"))
    check(2, ren, fresh("room", 70, 40, through), "room", planes + ("denoised",))
    ren.change_resolution(33, 17)                                               # every buffer shrinks; neither side is a multiple of 8
    check(3, ren, fresh("room", 33, 17, through), "room", planes + ("denoised", "despeckled", "motion", "chain"))
    assert ren.debug_guide_chain(1)[2].any()                                    # the mirror is in view: the chain's lists are in use
    ren.change_resolution(130, 70)                                              # more than one 64-pixel tile each way
    ren.set_guide_mode(*first_hit)
    ren.change_scene(scene("atrium"))
    one_device = fresh("atrium", 130, 70, first_hit)
    check(4, ren, one_device, "atrium", planes + ("denoised", "motion"))
    ren.set_devices([instance.device] * 2)                                      # the stage runs on device 0 after the exchange
    check(5, ren, one_device, "atrium", ("denoised",))


# ---------------------------------------------------------------------------------------------------------------------
# 6. nothing else moves
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("config", ["two_kernels", "path", "chains3"])
def test_post_reads_do_not_disturb_the_accumulation(instance, config):
    desc = small_atrium()

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
    b.read_aov(0)
    b.read_aov(1)
    b.read_denoised()
    b.step(17)
    assert np.array_equal(bits(a.read_hdr()), bits(b.read_hdr()))
    assert np.array_equal(bits(a.read_result()), bits(b.read_result()))
    assert a.stats().launches == b.stats().launches == 24


# ---------------------------------------------------------------------------------------------------------------------
# 7. end to end
# ---------------------------------------------------------------------------------------------------------------------
def test_read_denoised_is_the_host_filter_of_what_the_renderer_returns(instance):
    ren = glaze_amd.RayTraceRenderer.new(instance, glaze_amd.RayTraceScene.from_desc(instance, small_atrium()), 256, 144)
    ren.set_seed(3)
    ren.set_depth(4)
    ren.step(8)
    for params in ({},) + NON_DEFAULT + (dict(iterations=2),):
        ren.set_denoise(**params)
        den, img = ren.read_denoised(want_rgba8=True)
        want = glaze_amd.host_denoise(ren.read_result(), ren.read_aov(0), ren.read_aov(1), **params)
        assert np.array_equal(bits(den), bits(want)), params
        tm = np.zeros((144, 256, 4), np.uint8)
        abi.check(abi.lib().glz_debug_tonemap(instance._h, den.ctypes.data, 256 * 144, tm.ctypes.data))
        assert np.array_equal(img, tm)
    assert np.array_equal(ren.read_denoised(), den)                                  # float output alone
    with pytest.raises(glaze_amd.GlazeError) as e:
        ren.set_denoise(iterations=0)
    assert e.value.status == -4
    with pytest.raises(glaze_amd.GlazeError) as e:
        ren.read_aov(2)
    assert e.value.status == -4
    ren.set_partition(0, 2)
    with pytest.raises(glaze_amd.GlazeError) as e:
        ren.read_denoised()
    assert e.value.status == -4
    ren.read_aov(0)                                                                  # needs no accumulator: still works
    ren.change_resolution(100, 60)                                                   # the post buffers follow the resolution
    ren.set_partition(0, 1)
    ren.step(2)
    assert ren.read_denoised().shape == (60, 100, 4) and ren.read_aov(1).shape == (60, 100, 4)


@pytest.mark.skipif(not os.path.exists(CLI), reason="glaze-cli is not built")
def test_cli_denoise_writes_what_the_library_returns(tmp_path, instance):
    png, pfm, prefix = str(tmp_path / "o.png"), str(tmp_path / "o.pfm"), str(tmp_path / "aov")
    r = subprocess.run([CLI, MATTEST, png, "-r", "96x64", "-s", "3", "--seed", "11", "--depth", "4", "--denoise", "--hdr-out", pfm, "--aov-out", prefix],
                       capture_output=True, text=True)
    assert r.returncode == 0 and "All done :)" in r.stderr, r.stderr
    ren = glaze_amd.RayTraceRenderer.new(instance, glaze_amd.RayTraceScene.new(instance, glaze_amd.parse(MATTEST)), 96, 64)
    ren.set_seed(11)
    ren.set_depth(4)
    ren.draw(3, want_image=False)
    den, img = ren.read_denoised(want_rgba8=True)
    assert np.array_equal(np.asarray(Image.open(png)), img)
    with open(pfm, "rb") as f:
        assert f.readline() == b"PF\n" and f.readline() == b"96 64\n" and float(f.readline()) < 0
        data = np.frombuffer(f.read(), "<f4").reshape(64, 96, 3)[::-1]
    ok = np.isfinite(den[..., :3]).all(-1) & (den[..., 3] > 0)
    assert np.allclose(data[ok], den[..., :3][ok], rtol=1e-6, atol=0)
    nd, ai = ren.read_aov(0), ren.read_aov(1)
    assert np.array_equal(np.fromfile(prefix + ".depth.bin", "<f4").view(np.uint32), bits(nd[..., 3]).ravel())
    normal_png = np.asarray(Image.open(prefix + ".normal.png"))[..., :3]
    assert np.abs(normal_png.astype(np.float64) - (nd[..., :3] * 0.5 + 0.5) * 255.0).max() <= 0.5 + 1e-3
    albedo = ai.copy()
    albedo[..., 3] = 1.0
    tm = np.zeros((64, 96, 4), np.uint8)
    abi.check(abi.lib().glz_debug_tonemap(instance._h, np.ascontiguousarray(albedo).ctypes.data, 96 * 64, tm.ctypes.data))
    assert np.array_equal(np.asarray(Image.open(prefix + ".albedo.png"))[..., :3], tm[..., :3])


# ---------------------------------------------------------------------------------------------------------------------
# 8. it denoises
# ---------------------------------------------------------------------------------------------------------------------
def denoise_ratios(instance, desc, seed, converged):
    """(MSE ratio over all pixels finite in the three images, the same without the 1 % of pixels whose NOISY error is largest)"""
    ren = glaze_amd.RayTraceRenderer.new(instance, glaze_amd.RayTraceScene.from_desc(instance, desc), 256, 144)
    ren.set_depth(8)
    ren.set_seed(seed)
    ren.draw(2, want_image=False)
    noisy, den = ren.read_result()[..., :3].astype(np.float64), ren.read_denoised()[..., :3].astype(np.float64)
    ok = np.isfinite(noisy).all(-1) & np.isfinite(den).all(-1) & np.isfinite(converged).all(-1)
    e_noisy, e_den = ((noisy - converged) ** 2).sum(-1), ((den - converged) ** 2).sum(-1)
    keep = ok & (e_noisy <= np.quantile(e_noisy[ok], 0.99))
    return e_den[ok].mean() / e_noisy[ok].mean(), e_den[keep].mean() / e_noisy[keep].mean()


def converged_image(instance, desc):
    ren = glaze_amd.RayTraceRenderer.new(instance, glaze_amd.RayTraceScene.from_desc(instance, desc), 256, 144)
    ren.set_depth(8)
    ren.set_seed(987654321)
    ren.draw(512, want_image=False)
    return ren.read_result()[..., :3].astype(np.float64)


SEEDS = (1, 2, 3, 4, 5, 6, 7, 8)
# measured on an MI355X with the default parameters, seeds 1 .. 8 (see the docstring of test_it_denoises_a_render)
MEASURED = (0.9269, 0.9275, 0.9275, 0.9271, 0.9278, 0.9275, 0.9287, 0.9269)
MEASURED_TRIMMED = (0.3265, 0.3347, 0.3369, 0.3294, 0.3295, 0.3498, 0.3466, 0.3509)
GATE = (max(MEASURED) * 1.0) ** 0.5                    # 0.9637: halfway, in log terms, between the worst seed and no improvement
GATE_TRIMMED = (max(MEASURED_TRIMMED) * 1.0) ** 0.5    # 0.5923, by the same rule


def test_it_denoises_a_render(instance):
    """The small Sponza-like atrium at 256 x 144, depth 8, path tracer: noisy = 2 spp, converged = 512 spp of the existing, unfiltered
    path with another seed.  MSE(denoised, converged) / MSE(noisy, converged) over the pixels finite in all three must be below 1, and
    below the gate: the geometric mean of the worst measured seed's ratio and 1.

    Measured (MI355X, default parameters), seeds 1 .. 8: 0.9269, 0.9275, 0.9275, 0.9271, 0.9278, 0.9275, 0.9287, 0.9269 -> gate 0.9637.
    The ratio hardly moves with the seed because it is not the noisy image that sets it: 91 % of MSE(noisy, converged) sits in ten
    pixels at which the 512-spp REFERENCE still holds a firefly (up to 382 where the image's mean is 0.29), and no spatial filter of a
    2-spp image moves towards those.  Without the 1 % of pixels whose noisy error is largest (the same pixels dropped on both sides of the
    ratio) the eight seeds give 0.3265, 0.3347, 0.3369, 0.3294, 0.3295, 0.3498, 0.3466, 0.3509 -> gate 0.5923 by the same rule; that
    second figure is what the parameters were chosen on (tools/gpu_denoise_sweep.py, profiles/denoise_sweep.txt: with each parameter
    varied alone it stays within 0.31 .. 0.34, so the prototype's values were kept)."""
    desc = small_atrium()
    converged = converged_image(instance, desc)
    ratios = [denoise_ratios(instance, desc, s, converged) for s in SEEDS]
    print("MSE ratios over seeds %s: %s" % (SEEDS, ", ".join("%.4f" % r[0] for r in ratios)))
    print("  without the 1 %% largest noisy errors: %s" % ", ".join("%.4f" % r[1] for r in ratios))
    assert max(r[0] for r in ratios) < 1.0
    assert max(r[0] for r in ratios) < GATE
    assert max(r[1] for r in ratios) < GATE_TRIMMED
