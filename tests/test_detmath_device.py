"""include/glz_detmath.h: accuracy against float64 on the host, and the device build equal to the host build.

Both the kernels and the oracle include the header, so renders that agree bit for bit cannot see a mistake in it: its accuracy is
checked here against numpy's float64 functions on dense sweeps of the domains the renderer uses, glz_floorf for exactness on every
kind of float, and the device's code (glz_debug_detmath) against the host's value for value over a stride of all 2^32 bit patterns."""
import numpy as np
import pytest

from oracle import pyoracle

PI = np.pi
N = 1 << 23


def ulp_err(got, ref):
    """|got - ref| in units of the float32 spacing at ref"""
    return np.abs(got.astype(np.float64) - ref) / np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)


def strided_patterns(stride=251):
    """every float32 bit pattern at a prime stride over all 2^32 (about 1.7e7), plus the special values and the neighbourhoods of
    +-2^23, +-2^25 and +-2^31"""
    a = np.arange(0, 1 << 32, stride, dtype=np.uint64).astype(np.uint32).view(np.float32)
    near = []
    for p in (23, 25, 31):
        c = np.float32(2.0 ** p)
        b = c.view(np.uint32)
        near.append((b + np.arange(-300, 300, dtype=np.int64)).astype(np.uint32).view(np.float32))
        near.append(-near[-1])
        near.append(np.float32(c) + np.arange(-8, 8, dtype=np.float32) * np.float32(0.5))
    special = np.array([0.0, -0.0, 1e-45, -1e-45, 1.1754942e-38, 0.5, -0.5, 1.0, -1.0, 1.5, -1.5, 3e9, -3e9, 4e9, 1e20, -1e20,
                        3.4028235e38, -3.4028235e38, np.inf, -np.inf, np.nan], np.float32)
    return np.concatenate([a, special] + near)


# ---- accuracy on the host, over the renderer's domains ---------------------------------------------------------------------------
# Bounds measured on this code with a little headroom; the header states them.
def test_sin_cos_accuracy():
    x = np.linspace(-2 * PI, 2 * PI, N).astype(np.float32)
    x64 = x.astype(np.float64)
    assert ulp_err(pyoracle.detmath("sin", x), np.sin(x64)).max() <= 1.6
    c = pyoracle.detmath("cos", x)
    # cos is within 1e-7 absolute everywhere; its ulp error grows near its zeros (13.8 ulp at 3 pi / 2), so the ulp bound holds
    # where |cos| >= 1/8
    assert np.abs(c.astype(np.float64) - np.cos(x64)).max() <= 1.0e-7
    far = np.abs(np.cos(x64)) >= 0.125
    assert ulp_err(c[far], np.cos(x64[far])).max() <= 1.6


def test_acos_accuracy():
    x = np.concatenate([np.linspace(-1, 1, N), [-1.0, -0.5, 0.5, 1.0]]).astype(np.float32)
    assert ulp_err(pyoracle.detmath("acos", x), np.arccos(x.astype(np.float64))).max() <= 1.35
    assert pyoracle.detmath("acos", np.array([1.0, 1.5, -1.5], np.float32)).tolist() == [0.0, 0.0, np.float32(PI)]


def test_atan2_accuracy():
    rng = np.random.default_rng(3)
    y, x = rng.normal(size=N).astype(np.float32), rng.normal(size=N).astype(np.float32)
    # and every direction of the unit circle at a fine step
    t = np.linspace(-PI, PI, 1 << 20)
    y, x = np.concatenate([y, np.sin(t).astype(np.float32)]), np.concatenate([x, np.cos(t).astype(np.float32)])
    assert ulp_err(pyoracle.detmath("atan2", x, y), np.arctan2(y.astype(np.float64), x.astype(np.float64))).max() <= 3.5


def test_log2_accuracy():
    """every positive normal float at a stride of 127 bit patterns (1.7e7 values): the texture level of detail's log2"""
    x = np.arange(0x00800000, 0x7F800000, 127, dtype=np.uint32).view(np.float32)
    near_one = (np.int64(0x3F800000) + np.arange(-200000, 200000)).astype(np.uint32).view(np.float32)
    x = np.concatenate([x, near_one])
    ref = np.log2(x.astype(np.float64))
    got = pyoracle.detmath("log2", x)
    small = np.abs(ref) < 2 ** -10
    assert ulp_err(got[~small], ref[~small]).max() <= 2.0
    # next to 1, where log2 x -> 0: relative error
    assert (np.abs(got[small].astype(np.float64) - ref[small]) / np.abs(np.where(ref[small] == 0, 1, ref[small]))).max() <= 1.5e-7
    assert pyoracle.detmath("log2", np.array([1.0, 2.0, 0.5, 1024.0], np.float32)).tolist() == [0.0, 1.0, -1.0, 10.0]


def test_floor_is_exact_everywhere():
    """glz_floorf on a stride of every float32, huge values, +-inf and NaN: floor exactly (NaN for NaN; floor(-0) may be +0)"""
    x = strided_patterns()
    got = pyoracle.detmath("floor", x)
    with np.errstate(invalid="ignore"):
        ref = np.floor(x)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan)
    bad = got[~nan] != ref[~nan]
    assert not bad.any(), "glz_floorf wrong at %s: %s" % (x[~nan][bad][:6], got[~nan][bad][:6])


# ---- the device build equals the host build ------------------------------------------------------------------------------------
def assert_same(g, c, what):
    nan = np.isnan(c)
    assert np.array_equal(np.isnan(g), nan), what + ": NaN results differ"
    diff = g[~nan].view(np.uint32) != c[~nan].view(np.uint32)
    assert not diff.any(), "%s: %d values differ from the host" % (what, diff.sum())


@pytest.mark.gpu
@pytest.mark.parametrize("fn", ["sin", "cos", "acos", "log2", "floor"])
def test_device_detmath_equals_host(instance, fn):
    x = strided_patterns()
    assert_same(instance.debug_detmath(fn, x), pyoracle.detmath(fn, x), fn)


@pytest.mark.gpu
def test_device_floor_of_huge_values(instance):
    """what the device made of (float)(int)x outside +-2^31 (v_cvt_i32_f32 saturates) no longer matters: floor is x itself"""
    x = np.array([3e9, -3e9, 2.0 ** 31, -2.0 ** 31, 1e20, np.inf, -np.inf], np.float32)
    assert np.array_equal(instance.debug_detmath("floor", x), x)


@pytest.mark.gpu
def test_device_atan2_equals_host(instance):
    rng = np.random.default_rng(8)
    a = np.concatenate([rng.normal(size=2048) * np.exp(rng.uniform(-20, 20, 2048)), rng.uniform(-1, 1, 2048)]).astype(np.float32)
    b = rng.permutation(a)
    y, x = np.meshgrid(a, b)
    special = np.array([0.0, -0.0, 1e-45, -1e-45, 1.0, -1.0, 3.4028235e38, -3.4028235e38, np.inf, -np.inf, np.nan], np.float32)
    sy, sx = np.meshgrid(special, special)
    y, x = np.concatenate([y.ravel(), sy.ravel()]), np.concatenate([x.ravel(), sx.ravel()])
    assert_same(instance.debug_detmath("atan2", x, y), pyoracle.detmath("atan2", x, y), "atan2")
