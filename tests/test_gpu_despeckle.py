"""Firefly rejection on the device: k_despeckle against the host rule bit for bit (the host rule is checked against a float64
restatement of the specification in tests/test_despeckle_host.py), through the renderer (read_despeckled, read_denoised with the
rejection enabled), without disturbing a running accumulation, through the command line -- and that it helps a render.
"""
import os
import subprocess

import numpy as np
import pytest
from PIL import Image

import glaze_amd
from glaze_amd import abi
from glaze_amd.scenes import atrium_scene, mirror_room_scene

from conftest import MATTEST
from denoise_ref import synthetic_frame
from despeckle_ref import planted_frame

pytestmark = pytest.mark.gpu

CLI = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "glaze_amd", "csrc", "glaze-cli")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_same_bits(dev, host, what):
    differ = (bits(host) != bits(dev)).any(-1)
    assert not differ.any(), "%d pixels differ (%s), first at %s" % (differ.sum(), what, np.argwhere(differ)[0])


def speckled(width, height, seed):
    """a synthetic frame of any size with about 4 % of its pixels multiplied by 1e3 (clusters happen) and a NaN, a +inf and a -inf pixel"""
    result, aov0, aov1, _ = synthetic_frame(width, height, seed, spp=1)
    rng = np.random.default_rng(seed + 1000)
    result[..., :3] *= np.where(rng.random((height, width, 1)) < 0.04, np.float32(1e3), np.float32(1.0))
    flat = result.reshape(-1, 4)
    for j, v in zip(rng.choice(width * height, size=min(3, width * height), replace=False), (np.nan, np.inf, -np.inf)):
        if width * height > 3:
            flat[j, j % 3] = v
    return result, aov0, aov1


def tonemapped(instance, image):
    h, w = image.shape[:2]
    tm = np.zeros((h, w, 4), np.uint8)
    abi.check(abi.lib().glz_debug_tonemap(instance._h, np.ascontiguousarray(image).ctypes.data, w * h, tm.ctypes.data))
    return tm


# ---------------------------------------------------------------------------------------------------------------------
# device == host, bit for bit
# ---------------------------------------------------------------------------------------------------------------------
# the sizes cross a wave's 64-pixel edge and the block's 4-row edge, and include windows larger than the image
@pytest.mark.parametrize("size", [(1, 1), (2, 3), (63, 5), (67, 9), (130, 70)])
def test_device_rule_equals_host_rule(instance, size):
    result, aov0, aov1 = speckled(size[0], size[1], seed=size[0])
    for radius in (1, 2):
        for trim in (0, 3):
            for with_filter in (False, True):
                host = glaze_amd.host_despeckle(result, aov0, aov1, with_filter=with_filter, radius=radius, trim=trim)
                dev = instance.debug_despeckle(result, aov0, aov1, with_filter=with_filter, radius=radius, trim=trim)
                assert_same_bits(dev, host, "radius %d trim %d filter %s" % (radius, trim, with_filter))
    # non-default ratio and eps_albedo go the same way
    kw = dict(ratio=4.0, denoise=dict(eps_albedo=0.3, iterations=2))
    assert_same_bits(instance.debug_despeckle(result, aov0, aov1, **kw), glaze_amd.host_despeckle(result, aov0, aov1, **kw), "ratio 4")
    assert_same_bits(instance.debug_despeckle(result, aov0, aov1, with_filter=True, **kw), glaze_amd.host_despeckle(result, aov0, aov1, with_filter=True, **kw), "ratio 4, filter")


def test_device_rule_equals_host_rule_at_1080p(instance):
    result, aov0, aov1 = speckled(1920, 1080, seed=11)
    for kw in (dict(), dict(with_filter=True), dict(radius=1, trim=0), dict(radius=1, trim=3), dict(radius=2, trim=0), dict(radius=2, trim=3)):
        host = glaze_amd.host_despeckle(result, aov0, aov1, **kw)
        dev, ms = instance.debug_despeckle(result, aov0, aov1, want_ms=True, **kw)
        assert_same_bits(dev, host, kw)
        assert 0.0 < ms < 50.0                                       # the device-event time of k_despeckle alone
    untouched = glaze_amd.host_despeckle(result, aov0, aov1, ratio=3e38)
    assert (bits(untouched) != bits(glaze_amd.host_despeckle(result, aov0, aov1))).any(-1).sum() > 10000        # the rule had work to do


@pytest.mark.parametrize("size", [(150, 83), (97, 61)])
def test_device_rule_equals_host_rule_on_the_planted_frames(instance, size):
    for spp in (1, 4):
        for seed in (1, 2, 3):
            _, planted, aov0, aov1, _, _, _ = planted_frame(size[0], size[1], spp, seed)
            for radius in (1, 2):
                for trim in (0, 2):
                    host = glaze_amd.host_despeckle(planted, aov0, aov1, radius=radius, trim=trim)
                    dev = instance.debug_despeckle(planted, aov0, aov1, radius=radius, trim=trim)
                    assert_same_bits(dev, host, (spp, seed, radius, trim))
            assert_same_bits(instance.debug_despeckle(planted, aov0, aov1, with_filter=True), glaze_amd.host_despeckle(planted, aov0, aov1, with_filter=True), (spp, seed))


def test_bad_parameters_launch_nothing(instance):
    result, aov0, aov1 = speckled(32, 20, seed=2)
    for p in (dict(radius=0), dict(radius=3), dict(trim=4), dict(ratio=0.5), dict(ratio=np.nan), dict(ratio=np.inf), dict(with_filter=True, denoise=dict(iterations=9))):
        with pytest.raises(glaze_amd.GlazeError) as e:
            instance.debug_despeckle(result, aov0, aov1, **p)
        assert e.value.status == -4, p
    # without the filter only eps_albedo of the denoise parameters is read: the others cannot fail the call
    kw = dict(denoise=dict(iterations=0, sigma_color=-1.0, eps_albedo=0.3))
    assert_same_bits(instance.debug_despeckle(result, aov0, aov1, **kw), glaze_amd.host_despeckle(result, aov0, aov1, denoise=dict(eps_albedo=0.3)), "unused fields")


# ---------------------------------------------------------------------------------------------------------------------
# through the renderer
# ---------------------------------------------------------------------------------------------------------------------
def small_atrium():
    return atrium_scene(sponza_like=True, texture_size=64, sky_size=(64, 32))


@pytest.mark.parametrize("case", ["atrium", "mirror_room"])
def test_renderer_reads_equal_the_host_composition(instance, case):
    if case == "atrium":
        desc, w, h = small_atrium(), 256, 144
    else:
        desc, w, h = mirror_room_scene(), 128, 72
    ren = glaze_amd.RayTraceRenderer.new(instance, glaze_amd.RayTraceScene.from_desc(instance, desc), w, h)
    if case == "mirror_room":
        ren.set_guide_mode("through_specular")
    ren.set_seed(3)
    ren.set_depth(8)
    ren.draw(2, want_image=False)
    assert ren.despeckle() == (False, dict(radius=2, trim=2, ratio=8.0))
    result, aov0, aov1 = ren.read_result(), ren.read_aov(0), ren.read_aov(1)
    # the default state: read_denoised is the filter alone, as before
    den, img = ren.read_denoised(want_rgba8=True)
    assert_same_bits(den, glaze_amd.host_denoise(result, aov0, aov1), "disabled")
    assert np.array_equal(img, tonemapped(instance, den))
    # read_despeckled applies the rule whatever the flag says
    for params in (dict(), dict(radius=1, trim=1, ratio=4.0)):
        ren.set_despeckle(False, **params)
        out, img = ren.read_despeckled(want_rgba8=True)
        want = glaze_amd.host_despeckle(result, aov0, aov1, **params)
        assert_same_bits(out, want, params)
        assert np.array_equal(img, tonemapped(instance, out))
        assert_same_bits(ren.read_denoised(), den, "still disabled")
        ren.set_despeckle(True, **params)
        assert ren.despeckle() == (True, dict(dict(radius=2, trim=2, ratio=8.0), **params))
        both, img = ren.read_denoised(want_rgba8=True)
        assert_same_bits(both, glaze_amd.host_despeckle(result, aov0, aov1, with_filter=True, **params), params)
        assert np.array_equal(img, tonemapped(instance, both))
        assert_same_bits(ren.read_despeckled(), want, "enabled")
    assert (bits(out) != bits(result)).any(-1).sum() > 0 and (bits(both) != bits(den)).any(-1).sum() > 0      # the rule had work to do
    # the denoiser's parameters in force are the ones the composition uses
    ren.set_denoise(iterations=2, eps_albedo=0.05)
    ren.set_despeckle(True)
    assert_same_bits(ren.read_denoised(), glaze_amd.host_despeckle(result, aov0, aov1, with_filter=True, denoise=dict(iterations=2, eps_albedo=0.05)), "denoise params")
    assert_same_bits(ren.read_despeckled(), glaze_amd.host_despeckle(result, aov0, aov1, denoise=dict(eps_albedo=0.05)), "eps_albedo")
    # bad parameters change nothing
    for p in (dict(radius=0), dict(radius=3), dict(trim=4), dict(ratio=0.5), dict(ratio=np.nan), dict(ratio=np.inf)):
        with pytest.raises(glaze_amd.GlazeError) as e:
            ren.set_despeckle(False, **p)
        assert e.value.status == -4, p
    assert ren.despeckle() == (True, dict(radius=2, trim=2, ratio=8.0))
    assert abi.lib().glz_renderer_set_despeckle(ren._h, 1, None) == 0 and abi.lib().glz_renderer_despeckle(ren._h, None) == 1      # NULL = defaults; out may be NULL


@pytest.mark.parametrize("config", ["two_kernels", "path", "chains3"])
def test_despeckle_reads_do_not_disturb_the_accumulation(instance, config):
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
    b.set_despeckle(True, ratio=4.0)
    b.read_despeckled()
    b.read_denoised()
    b.step(9)
    b.set_despeckle(False)
    b.read_despeckled(want_rgba8=True)
    b.step(8)
    assert np.array_equal(bits(a.read_hdr()), bits(b.read_hdr()))
    assert np.array_equal(bits(a.read_result()), bits(b.read_result()))
    assert a.stats().launches == b.stats().launches == 24


def test_partition_and_devices(instance, monkeypatch):
    monkeypatch.setenv("GLAZE_MULTI_LOOPBACK", "1")
    desc = small_atrium()

    def renderer():
        r = glaze_amd.RayTraceRenderer.new(instance, glaze_amd.RayTraceScene.from_desc(instance, desc), 150, 83)
        r.set_seed(5)
        r.set_depth(4)
        return r

    one = renderer()
    one.step(3)
    want = one.read_despeckled()
    two = renderer()
    two.set_devices([instance.device] * 2)
    two.step(3)
    assert_same_bits(two.read_despeckled(), want, "set_devices, n = 2")        # device 0 after the exchange
    two.set_despeckle(True)
    one.set_despeckle(True)
    assert_same_bits(two.read_denoised(), one.read_denoised(), "set_devices, n = 2, with the filter")
    one.set_partition(0, 2)
    with pytest.raises(glaze_amd.GlazeError) as e:
        one.read_despeckled()
    assert e.value.status == -4
    assert one.despeckle()[0] is True


@pytest.mark.skipif(not os.path.exists(CLI), reason="glaze-cli is not built")
@pytest.mark.parametrize("denoise", [False, True])
def test_cli_despeckle_writes_what_the_library_returns(tmp_path, instance, denoise):
    png, pfm = str(tmp_path / "o.png"), str(tmp_path / "o.pfm")
    r = subprocess.run([CLI, MATTEST, png, "-r", "96x64", "-s", "3", "--seed", "11", "--depth", "4", "--despeckle-ratio", "2.5", "--hdr-out", pfm]
                       + (["--denoise"] if denoise else []), capture_output=True, text=True)
    assert r.returncode == 0 and "All done :)" in r.stderr, r.stderr
    ren = glaze_amd.RayTraceRenderer.new(instance, glaze_amd.RayTraceScene.new(instance, glaze_amd.parse(MATTEST)), 96, 64)
    ren.set_seed(11)
    ren.set_depth(4)
    ren.draw(3, want_image=False)
    ren.set_despeckle(True, ratio=2.5)
    out, img = ren.read_denoised(want_rgba8=True) if denoise else ren.read_despeckled(want_rgba8=True)
    assert (bits(out) != bits(ren.read_result())).any(-1).sum() > 0
    assert np.array_equal(np.asarray(Image.open(png)), img)
    with open(pfm, "rb") as f:
        assert f.readline() == b"PF\n" and f.readline() == b"96 64\n" and float(f.readline()) < 0
        data = np.frombuffer(f.read(), "<f4").reshape(64, 96, 3)[::-1]
    ok = np.isfinite(out[..., :3]).all(-1) & (out[..., 3] > 0)
    assert np.allclose(data[ok], out[..., :3][ok], rtol=1e-6, atol=0)
    if not denoise:                                                   # --despeckle alone takes the default ratio
        r = subprocess.run([CLI, MATTEST, png, "-r", "96x64", "-s", "3", "--seed", "11", "--depth", "4", "--despeckle"], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        ren.set_despeckle(True)
        assert np.array_equal(np.asarray(Image.open(png)), ren.read_despeckled(want_rgba8=True)[1])


# ---------------------------------------------------------------------------------------------------------------------
# it helps a render
# ---------------------------------------------------------------------------------------------------------------------
SEEDS = (1, 2, 3, 4, 5, 6, 7, 8)
REFERENCE_SEEDS = tuple(range(101, 110))
# measured on an MI355X with the default parameters, seeds 1 .. 8 (see the docstring of test_rejection_helps_the_denoised_render)
MEASURED = (0.8699, 0.8837, 0.8630, 0.8671, 0.8635, 0.4829, 0.8757, 0.8273)
GATE = (max(MEASURED) * 1.0) ** 0.5                    # 0.9401: halfway, in log terms, between the worst seed and no improvement


def render(instance, desc, seed, spp):
    ren = glaze_amd.RayTraceRenderer.new(instance, glaze_amd.RayTraceScene.from_desc(instance, desc), 256, 144)
    ren.set_depth(8)
    ren.set_seed(seed)
    ren.draw(spp, want_image=False)
    return ren


def median_reference(instance, desc):
    """per pixel and channel, the median of nine independent 64-spp renders: a median of means does not keep a firefly the way the single
    512-spp image of test_gpu_denoise.py does (there 91 % of MSE(noisy, converged) sits in ten pixels of the REFERENCE)"""
    return np.median(np.stack([render(instance, desc, s, 64).read_result()[..., :3].astype(np.float64) for s in REFERENCE_SEEDS]), axis=0)


def rejection_ratio(instance, desc, seed, reference):
    ren = render(instance, desc, seed, 2)
    without = ren.read_denoised()[..., :3].astype(np.float64)
    ren.set_despeckle(True)
    with_it = ren.read_denoised()[..., :3].astype(np.float64)
    return ((with_it - reference) ** 2).mean() / ((without - reference) ** 2).mean()


def test_rejection_helps_the_denoised_render(instance):
    """The small Sponza-like atrium at 256 x 144, depth 8, path tracer.  The reference R is the per-pixel, per-channel median of nine
    independent 64-spp renders (seeds 101 .. 109): a median of means does not keep a firefly the way the single 512-spp image of
    test_gpu_denoise.py does (R: max 2.98, mean 0.271; the 512-spp image: max 382.5, mean 0.288 -- the median also sits below the mean
    of a skewed estimator, so R leans towards whatever removes energy; the figures below are to be read with that in mind).  For seeds
    1 .. 8 at 2 spp: MSE(read_denoised with the rejection, R) / MSE(read_denoised without, R) over all pixels, nothing trimmed, must be
    below the gate, the geometric mean of the worst measured seed's ratio and 1.

    Measured (MI355X, default parameters), seeds 1 .. 8: 0.8699, 0.8837, 0.8630, 0.8671, 0.8635, 0.4829, 0.8757, 0.8273 -> gate 0.9401.
    (Seed 6 holds one firefly the filter spreads: MSE(filter alone, R) is 0.167 there against 0.083 .. 0.091 for the others.)  Without a
    gate (tools/gpu_denoise_sweep.py, profiles/despeckle_sweep.txt): against the 512-spp image, seed 1, rejection + filter gives 0.9247
    over all pixels and 0.2860 without the 1 % largest noisy errors (the filter alone: 0.9269 and 0.3265); the rule clamps 5.04 % of
    the hit pixels at 2 spp and 0.68 % at 512 spp; mean(despeckled) / mean(result) is 0.9442 at 2 spp and 0.9529 at 512 spp -- the energy
    it removes."""
    desc = small_atrium()
    reference = median_reference(instance, desc)
    assert np.isfinite(reference).all()
    ratios = [rejection_ratio(instance, desc, s, reference) for s in SEEDS]
    print("MSE(read_denoised with rejection, R) / MSE(read_denoised without, R) over seeds %s: %s" % (SEEDS, ", ".join("%.4f" % r for r in ratios)))
    assert max(ratios) < GATE
