"""The firefly rejection on the host (glz_host_despeckle: the reference k_despeckle must match bit for bit) and its command line.
CPU only.

The rule is specified in the header comment of glz_despeckle_params (include/glaze_abi.h); tests/despeckle_ref.py restates that comment
in float64 numpy.  Unlike the filter's weights the rule has a threshold, so the comparison first makes sure that no decision of these
frames sits on a rounding (the restatement's nearest |L / T - 1| is far above float32's 6e-8), then asks for the same SET of clamped
pixels and compares the values.
"""
import os
import subprocess

import numpy as np
import pytest

import glaze_amd
from glaze_amd import abi

from denoise_ref import synthetic_frame
from despeckle_ref import planted_frame, reference_despeckle

CLI = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "glaze_amd", "csrc", "glaze-cli")
MATTEST = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mattest.glaze")
EPS_A = np.float32(1.0 / 256.0)

# Host (binary32) against the float64 restatement, relative, on the frames of test_host_matches_the_float64_restatement: four times the
# largest error measured there, 3.31e-7 (a 24-term sum of positive terms, a quotient and two products, one more quotient and product
# for the albedo: of the order of 1e-6 in the worst case, about five roundings of 2^-24 = 6e-8 as measured).
VALUE_BOUND = 4 * 3.31e-7


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def plain(result, aov1):
    """demodulate and re-modulate, in binary32: what the rejection returns for a pixel it leaves alone"""
    with np.errstate(all="ignore"):
        A = np.where(aov1[..., :3] > EPS_A, aov1[..., :3], EPS_A).astype(np.float32)
        out = result.copy()
        out[..., :3] = (result[..., :3] / A) * A
    return out


def same(a, b):
    """equal by bits, any NaN equal to any NaN"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))


def changed(out, result, aov1):
    base = plain(result, aov1)
    return ~np.all((bits(out) == bits(base)) | (np.isnan(out) & np.isnan(base)), -1)


@pytest.mark.parametrize("size", [(150, 83), (97, 61)])
@pytest.mark.parametrize("spp", [1, 4])
def test_host_matches_the_float64_restatement(size, spp):
    worst, nearest_of_all = 0.0, np.inf
    for seed in (1, 2, 3):
        _, planted, aov0, aov1, _, spots, bad = planted_frame(size[0], size[1], spp, seed)
        for radius in (1, 2):
            for trim in (0, 2):
                got = glaze_amd.host_despeckle(planted, aov0, aov1, radius=radius, trim=trim)
                want, clamped, _, nearest = reference_despeckle(planted, aov0, aov1, radius=radius, trim=trim)
                nearest_of_all = min(nearest_of_all, nearest)
                assert nearest > 1e-3, (seed, radius, trim, nearest)          # no verdict of this frame sits on a rounding
                assert np.array_equal(changed(got, planted, aov1), clamped), (seed, radius, trim)     # the same set, no pixel excluded
                assert clamped.sum() >= 38                                   # (trim 0 loses the adjacent pair, by design)
                fin = np.isfinite(want[..., :3])
                assert np.array_equal(fin, np.isfinite(got[..., :3]))
                assert (want[..., :3][fin] != 0).all()                       # the relative error has a denominator everywhere
                err = np.abs(got[..., :3][fin] - want[..., :3][fin]) / np.abs(want[..., :3][fin])
                assert not np.isnan(err).any()
                worst = max(worst, err.max())
                assert np.array_equal(bits(got[..., 3]), bits(planted[..., 3]))
                for y, x in bad:                                             # the non-finite pixels pass through
                    assert same(got[y, x], plain(planted, aov1)[y, x])
    print("host vs float64: largest relative error %.3g, nearest |L/T - 1| %.3g" % (worst, nearest_of_all))
    assert worst <= VALUE_BOUND


def test_a_constant_frame_is_unchanged():
    result, aov0, aov1, _ = synthetic_frame(150, 83, seed=1, irradiance=0.7)
    # i_0 = 1/2 exactly at every hit (a power of two times A divides back exactly): L = 3/2, every partial sum is exact, mu = L
    result[..., :3] = np.where(np.isfinite(aov0[..., 3:4]), np.float32(0.5) * np.where(aov1[..., :3] > EPS_A, aov1[..., :3], EPS_A), result[..., :3])
    for radius in (1, 2):
        for trim in (0, 3):
            out = glaze_amd.host_despeckle(result, aov0, aov1, radius=radius, trim=trim, ratio=1.0)     # ratio 1: L = mu = T, not above it
            assert same(out, plain(result, aov1))


@pytest.mark.parametrize("k", [-20, 20])
def test_scaling_by_a_power_of_two_is_exact(k):
    _, planted, aov0, aov1, _, _, _ = planted_frame(97, 61, 1, 2)
    base = glaze_amd.host_despeckle(planted, aov0, aov1)
    scaled = planted.copy()
    scaled[..., :3] *= np.float32(2.0 ** k)
    out = glaze_amd.host_despeckle(scaled, aov0, aov1)
    want = base.copy()
    want[..., :3] *= np.float32(2.0 ** k)
    assert same(out, want)
    assert changed(out, scaled, aov1).sum() >= 40


def test_misses_and_non_finite_pixels_pass_through_and_only_drop_out_of_windows():
    result, planted, aov0, aov1, region, spots, bad = planted_frame(150, 83, 4, 1)
    out = glaze_amd.host_despeckle(planted, aov0, aov1)
    assert np.array_equal(bits(out[region == 0]), bits(planted[region == 0]))       # misses: albedo 1, back as they went in
    base = plain(planted, aov1)
    for y, x in bad:
        assert same(out[y, x], base[y, x])
    # a non-finite pixel changes no neighbour's verdict beyond dropping out of its window: the same frame with that pixel turned into a
    # miss (which drops out of every window too) gives every other pixel the same bits
    as_miss, aov0_m = planted.copy(), aov0.copy()
    for y, x in bad:
        as_miss[y, x, :3] = 1.0
        aov0_m[y, x, 3] = np.inf
    out_m = glaze_amd.host_despeckle(as_miss, aov0_m, aov1)
    others = np.ones(region.shape, bool)
    for y, x in bad:
        others[y, x] = False
    assert np.array_equal(bits(out[others]), bits(out_m[others]))
    # and it is never anybody's outlier: nothing but the planted pixels moves
    moved = changed(out, planted, aov1)
    want = np.zeros(region.shape, bool)
    for y, x in spots:
        want[y, x] = True
    assert np.array_equal(moved, want)


def test_the_sky_reaches_no_hit():
    _, planted, aov0, aov1, region, _, _ = planted_frame(150, 83, 1, 3)
    base = glaze_amd.host_despeckle(planted, aov0, aov1)
    scaled = planted.copy()
    scaled[region == 0, :3] *= np.float32(7.0)
    out = glaze_amd.host_despeckle(scaled, aov0, aov1)
    assert same(out[region != 0], base[region != 0])
    assert np.array_equal(bits(out[region == 0]), bits(scaled[region == 0]))


def test_a_lone_outlier_comes_back_at_its_threshold():
    result, aov0, aov1, region = synthetic_frame(150, 83, seed=5, spp=4)
    y, x = 62, 75                                                  # inside the floor
    lone = result.copy()
    lone[y, x, :3] = np.float32(1e30) * np.where(aov1[y, x, :3] > EPS_A, aov1[y, x, :3], EPS_A)
    out = glaze_amd.host_despeckle(lone, aov0, aov1)
    moved = changed(out, lone, aov1)
    assert moved.sum() == 1 and moved[y, x]
    _, clamped, over, _ = reference_despeckle(lone, aov0, aov1)
    T = 3e30 / over[y, x]                                          # L(p) / (L / T) in float64
    A = np.where(aov1[y, x, :3] > EPS_A, aov1[y, x, :3], EPS_A).astype(np.float64)
    L_out = (out[y, x, :3].astype(np.float64) / A).sum()
    print("lone outlier: L' / T - 1 = %.3g" % (L_out / T - 1))
    assert abs(L_out / T - 1) <= VALUE_BOUND


@pytest.mark.parametrize("trim", [0, 1, 2, 3])
def test_trim_adjacent_outliers_are_removed_and_trim_plus_one_survive(trim):
    """Counted as the rule counts them, in the window of the pixel in question (q != p): a firefly with `trim` fireflies among its
    neighbours is brought down to its surroundings, M being an ordinary value; with trim + 1 of them M is a firefly's L and it stays one
    (T >= (trim + 1) * ratio / 24 of its L, a third at the least).  The clusters lie inside a 3 x 3 block, so at radius 2 every member
    has all the others in its window."""
    result, aov0, aov1, _ = synthetic_frame(150, 83, seed=6, spp=4)
    cells = [(60 + j // 3, 70 + j % 3) for j in range(9)]
    A = np.where(aov1[..., :3] > EPS_A, aov1[..., :3], EPS_A)
    L_in = (result[..., :3] / A).sum(-1)
    ordinary = L_in[56:68, 66:78].max()
    for neighbours, survive in ((trim, False), (trim + 1, True)):
        planted = result.copy()
        for y, x in cells[:neighbours + 1]:
            planted[y, x, :3] = np.float32(1e4) * A[y, x]          # L = 3e4 each, against an ordinary level of about 3
        out = glaze_amd.host_despeckle(planted, aov0, aov1, trim=trim)
        L_out = (out[..., :3] / A).sum(-1)
        for y, x in cells[:neighbours + 1]:
            if survive:
                assert L_out[y, x] >= 3e4 / 4, (trim, neighbours, L_out[y, x])
            else:
                assert L_out[y, x] <= 8.0 * ordinary * (1 + 1e-6), (trim, neighbours, L_out[y, x])
        moved = changed(out, planted, aov1)
        for y, x in cells[:neighbours + 1]:
            moved[y, x] = False
        assert not moved.any()                                     # and nothing else in the frame moves


def compare_with_the_restatement(got, result, aov0, aov1, **params):
    """the same set of clamped pixels as the float64 restatement, no verdict on a rounding, values within VALUE_BOUND; returns the set"""
    want, clamped, _, nearest = reference_despeckle(result, aov0, aov1, **params)
    assert nearest > 1e-3, (params, nearest)
    assert np.array_equal(changed(got, result, aov1), clamped), params
    fin = np.isfinite(want[..., :3])
    assert np.array_equal(fin, np.isfinite(got[..., :3]))
    assert (want[..., :3][fin] != 0).all()                         # the relative error below has a denominator everywhere
    err = np.abs(got[..., :3][fin] - want[..., :3][fin]) / np.abs(want[..., :3][fin])
    assert not np.isnan(err).any() and (err.size == 0 or err.max() <= VALUE_BOUND), params
    return clamped


@pytest.mark.parametrize("size", [(1, 1), (2, 3), (5, 1)])
def test_frames_smaller_than_the_window(size):
    """Windows larger than the image.  Every pixel is a usable hit, so m is the number of window positions inside the image, counted here
    by hand: wherever m <= trim the pixel must come back unchanged by bits, and the rest must agree with the float64 restatement.
    1 x 1: m = 0 everywhere.  5 x 1 at radius 1: m <= 2, so trim 2 and 3 leave the whole frame alone; at radius 2 the end pixels have
    m = 2.  2 x 3: the corners have m = 3 at radius 1 (trim 3 leaves them alone), every pixel has m = 5 at radius 2.  One pixel is made
    an outlier so that the rule has work wherever it may act."""
    w, h = size
    rng = np.random.default_rng(w * 10 + h)
    result = rng.uniform(1.0, 2.0, size=(h, w, 4)).astype(np.float32)
    result[h // 2, w // 2, :3] *= np.float32(1e3)
    aov0 = np.zeros((h, w, 4), np.float32)
    aov0[..., 2] = 1.0
    aov0[..., 3] = 5.0
    aov1 = np.full((h, w, 4), 0.5, np.float32)
    base = plain(result, aov1)
    y, x = np.mgrid[0:h, 0:w]
    acted = 0
    for radius in (1, 2):
        m = (np.minimum(x + radius, w - 1) - np.maximum(x - radius, 0) + 1) * (np.minimum(y + radius, h - 1) - np.maximum(y - radius, 0) + 1) - 1
        for trim in (0, 1, 2, 3):
            for ratio in (1.25, 8.0):
                p = dict(radius=radius, trim=trim, ratio=ratio)
                out = glaze_amd.host_despeckle(result, aov0, aov1, **p)
                alone = m <= trim
                assert same(out[alone], base[alone]), p
                clamped = compare_with_the_restatement(out, result, aov0, aov1, **p)
                assert not (clamped & alone).any()
                acted += clamped.sum()
                if size == (1, 1) or (size == (5, 1) and radius == 1 and trim >= 2):
                    assert alone.all() and same(out, base), p
                if size == (5, 1) and radius == 2 and trim == 2:
                    assert alone[0, 0] and alone[0, 4] and not alone[0, 1:4].any()
                if size == (2, 3) and radius == 1 and trim == 3:
                    assert alone[0, 0] and alone[0, 1] and alone[2, 0] and alone[2, 1] and not alone[1].any()
    assert acted > 0 or size == (1, 1)


@pytest.mark.parametrize("spp", [1, 2, 4, 16])
def test_a_frame_without_outliers_is_left_alone(spp):
    largest = 0.0
    for seed in range(1, 9):
        result, aov0, aov1, _ = synthetic_frame(150, 83, seed, spp=spp)
        out = glaze_amd.host_despeckle(result, aov0, aov1)
        assert same(out, plain(result, aov1)), seed
        _, clamped, over, _ = reference_despeckle(result, aov0, aov1)
        assert not clamped.any()
        largest = max(largest, 8.0 * np.nanmax(over))
    print("spp %d: largest L / mu = %.3g against the ratio 8" % (spp, largest))


def mse(a, b):
    return float(((a[..., :3].astype(np.float64) - b[..., :3].astype(np.float64)) ** 2).mean())


@pytest.mark.parametrize("spp", [1, 2, 4, 16])
def test_it_does_its_job(spp):
    for seed in (1, 2, 3):
        result, planted, aov0, aov1, _, _, _ = planted_frame(150, 83, spp, seed, with_non_finite=False)
        truth = synthetic_frame(150, 83, seed, spp=4000)[0]        # the same frame all but converged, as test_denoise_host.py takes it
        clean = mse(glaze_amd.host_denoise(result, aov0, aov1), truth)
        both = mse(glaze_amd.host_despeckle(planted, aov0, aov1, with_filter=True), truth)
        alone = mse(glaze_amd.host_denoise(planted, aov0, aov1), truth)
        print("spp %d seed %d: MSE filter, no outliers %.4g; rejection + filter, planted %.4g (%.3f x); filter alone, planted %.4g (%.3g x)"
              % (spp, seed, clean, both, both / clean, alone, alone / clean))
        assert both <= 1.25 * clean
        assert alone >= 1e4 * clean


def test_bad_parameters_are_argument_errors():
    result, aov0, aov1, _ = synthetic_frame(32, 20, seed=2)
    for p in (dict(radius=0), dict(radius=3), dict(trim=4), dict(ratio=0.5), dict(ratio=np.nan), dict(ratio=np.inf)):
        for with_filter in (False, True):
            with pytest.raises(glaze_amd.GlazeError) as e:
                glaze_amd.host_despeckle(result, aov0, aov1, with_filter=with_filter, **p)
            assert e.value.status == -4, p                         # GLZ_E_ARG
    with pytest.raises(glaze_amd.GlazeError) as e:
        glaze_amd.host_despeckle(result, aov0, aov1, with_filter=True, denoise=dict(iterations=0))
    assert e.value.status == -4
    # without the filter only eps_albedo of the denoise parameters is read: the others cannot fail the call
    assert same(glaze_amd.host_despeckle(result, aov0, aov1, denoise=dict(iterations=0, sigma_depth=np.nan, eps_albedo=0.3)),
                glaze_amd.host_despeckle(result, aov0, aov1, denoise=dict(eps_albedo=0.3)))
    for p in (dict(radius=1, trim=0, ratio=1.0), dict(radius=2, trim=3, ratio=3e38)):
        assert glaze_amd.host_despeckle(result, aov0, aov1, **p).shape == result.shape
    assert abi.lib().glz_host_despeckle(32, 20, None, None, None, None, None, 0, None) == -4
    with pytest.raises(TypeError):
        abi.DespeckleParams(sigma=1.0)
    # NULL parameters are the defaults
    out = np.zeros_like(result)
    ptr = lambda a: a.ctypes.data_as(abi.C.c_void_p)
    assert abi.lib().glz_host_despeckle(32, 20, ptr(result), ptr(aov0), ptr(aov1), None, None, 0, ptr(out)) == 0
    assert same(out, glaze_amd.host_despeckle(result, aov0, aov1))


@pytest.mark.skipif(not os.path.exists(CLI), reason="glaze-cli is not built")
def test_cli_knows_the_despeckle_options(tmp_path):
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True)
    text = r.stdout + r.stderr
    assert r.returncode == 0 and "--despeckle " in text and "--despeckle-ratio" in text
    for bad in ("0.5", "nan", "inf", "eight", "8x", ""):
        r = subprocess.run([CLI, MATTEST, str(tmp_path / "o.png"), "--despeckle-ratio", bad], capture_output=True, text=True)
        assert r.returncode == 2 and "invalid value '%s' for '--despeckle-ratio'" % bad in r.stderr, bad
    r = subprocess.run([CLI, MATTEST, str(tmp_path / "o.png"), "--despeckle-ratio"], capture_output=True, text=True)
    assert r.returncode == 2 and "value is required" in r.stderr
