"""The denoiser's filter on the host (glz_host_denoise: the reference the device kernels must match bit for bit) and the command line
of the post features.  CPU only.

The filter is specified in the header comment of glz_denoise_params (include/glaze_abi.h); tests/denoise_ref.py restates that comment
in float64 numpy.  Its weights are continuous in the inputs, so float32 rounding cannot flip a tap; the tolerance of the comparison is
the project's own for small frames: rel <= 1e-4 on >= 99.9 % of the values, mean <= 1e-5.
"""
import os
import subprocess

import numpy as np
import pytest

import glaze_amd
from glaze_amd import abi

from denoise_ref import reference_denoise, synthetic_frame
from helpers import rel_err

CLI = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "glaze_amd", "csrc", "glaze-cli")
MATTEST = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mattest.glaze")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("size", [(150, 83), (97, 61)])
@pytest.mark.parametrize("iterations", [1, 3, 5])
def test_host_filter_matches_the_float64_restatement(size, iterations):
    result, aov0, aov1, _ = synthetic_frame(size[0], size[1], seed=iterations * 100 + size[0])
    got = glaze_amd.host_denoise(result, aov0, aov1, iterations=iterations)
    want = reference_denoise(result, aov0, aov1, iterations=iterations)
    assert np.isfinite(got).all()
    err = rel_err(got[..., :3], want[..., :3])
    print("host vs float64: max %.3g mean %.3g, within 1e-4: %.5f" % (err.max(), err.mean(), (err <= 1e-4).mean()))
    assert (err <= 1e-4).mean() >= 0.999 and err.mean() <= 1e-5
    assert np.array_equal(got[..., 3], result[..., 3])
    # non-default parameters go the same way
    p = dict(iterations=iterations, sigma_color=1.5, sigma_depth=0.25, normal_power_log2=3, eps_albedo=0.05, eps_depth=1e-2, eps_color=1e-4)
    err = rel_err(glaze_amd.host_denoise(result, aov0, aov1, **p)[..., :3], reference_denoise(result, aov0, aov1, **p)[..., :3])
    assert (err <= 1e-4).mean() >= 0.999 and err.mean() <= 1e-5


def test_it_denoises_the_synthetic_frame():
    result, aov0, aov1, _ = synthetic_frame(150, 83, seed=7)
    clean = synthetic_frame(150, 83, seed=7, spp=4000)[0]          # the same frame all but converged
    out = glaze_amd.host_denoise(result, aov0, aov1)
    mse_in = ((result[..., :3] - clean[..., :3]).astype(np.float64) ** 2).mean()
    mse_out = ((out[..., :3] - clean[..., :3]).astype(np.float64) ** 2).mean()
    print("MSE out / in = %.4f" % (mse_out / mse_in))
    assert mse_out < 0.5 * mse_in


def test_constant_irradiance_stays_constant():
    # out = c within 4e-6 relative: 25 rounded additions each in numerator and denominator at 2^-24, the divisions and the two
    # albedo multiplications
    result, aov0, aov1, _ = synthetic_frame(150, 83, seed=1, irradiance=0.7)
    out = glaze_amd.host_denoise(result, aov0, aov1)
    rel = np.abs(out[..., :3].astype(np.float64) - result[..., :3]) / result[..., :3]
    print("constant irradiance: max relative deviation %.3g" % rel.max())
    assert rel.max() <= 4e-6


@pytest.mark.parametrize("iterations", [1, 5])
def test_edges_separate_exactly(iterations):
    result, aov0, aov1, region = synthetic_frame(150, 83, seed=3)
    base = glaze_amd.host_denoise(result, aov0, aov1, iterations=iterations)
    # the floor's normal is perpendicular to the wall's: colours of the floor cannot reach the wall or the sky
    scaled = result.copy()
    scaled[region == 2, :3] *= 7.0
    out = glaze_amd.host_denoise(scaled, aov0, aov1, iterations=iterations)
    assert np.array_equal(bits(out[region != 2]), bits(base[region != 2]))
    assert not np.array_equal(out[region == 2], base[region == 2])
    # the hit / miss boundary: colours of the sky cannot reach a hit
    scaled = result.copy()
    scaled[region == 0, :3] *= 7.0
    out = glaze_amd.host_denoise(scaled, aov0, aov1, iterations=iterations)
    assert np.array_equal(bits(out[region != 0]), bits(base[region != 0]))
    assert not np.array_equal(out[region == 0], base[region == 0])


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_one_non_finite_pixel_is_filled_and_stays_local(bad):
    K = 3
    result, aov0, aov1, _ = synthetic_frame(150, 83, seed=5)
    base = glaze_amd.host_denoise(result, aov0, aov1, iterations=K)
    by, bx = 62, 75                                               # inside the floor
    broken = result.copy()
    broken[by, bx, 1] = bad
    out = glaze_amd.host_denoise(broken, aov0, aov1, iterations=K)
    assert np.isfinite(out).all() and np.isnan(out).sum() == 0
    y, x = np.mgrid[0:83, 0:150]
    far = np.maximum(np.abs(y - by), np.abs(x - bx)) > 2 * (2 ** K - 1)
    assert np.array_equal(bits(out[far]), bits(base[far]))
    assert np.array_equal(out[..., 3], result[..., 3])


def test_nothing_invents_a_value():
    result, aov0, aov1, _ = synthetic_frame(64, 40, seed=9)
    for bad in (np.nan, np.inf):
        broken = result.copy()
        broken[..., :3] = bad
        out = glaze_amd.host_denoise(broken, aov0, aov1)
        assert not np.isfinite(out[..., :3]).all(-1).any()


def test_bad_parameters_are_argument_errors():
    result, aov0, aov1, _ = synthetic_frame(32, 20, seed=2)
    for p in (dict(iterations=0), dict(iterations=9), dict(sigma_color=0.0), dict(sigma_color=-1.0), dict(sigma_color=np.nan),
              dict(sigma_color=np.inf), dict(sigma_depth=0.0), dict(sigma_depth=np.nan), dict(sigma_depth=-np.inf),
              dict(normal_power_log2=32), dict(normal_power_log2=1 << 24), dict(normal_power_log2=0xFFFFFFFF)):     # a loop's trip count in every tap
        with pytest.raises(glaze_amd.GlazeError) as e:
            glaze_amd.host_denoise(result, aov0, aov1, **p)
        assert e.value.status == -4, p                             # GLZ_E_ARG
    for it in (1, 8):
        assert glaze_amd.host_denoise(result, aov0, aov1, iterations=it).shape == result.shape
    # 31 squarings are the most that can matter: every float below 1 is 0 after them, so 31 and 30 differ at most where the cosine is 1
    assert np.isfinite(glaze_amd.host_denoise(result, aov0, aov1, normal_power_log2=31)).all()
    lib = abi.lib()
    assert lib.glz_host_denoise(32, 20, None, None, None, None, None) == -4
    with pytest.raises(TypeError):
        abi.DenoiseParams(sigma=1.0)


@pytest.mark.skipif(not os.path.exists(CLI), reason="glaze-cli is not built")
def test_cli_knows_the_post_options(tmp_path):
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True)
    text = r.stdout + r.stderr
    assert r.returncode == 0 and "--denoise" in text and "--aov-out" in text
    r = subprocess.run([CLI, MATTEST, str(tmp_path / "o.png"), "--aov-out"], capture_output=True, text=True)
    assert r.returncode == 2 and "value is required" in r.stderr
