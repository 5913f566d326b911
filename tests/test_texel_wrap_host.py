"""The texel index of a REPEAT texture (device/shading.h bilinear_level; glz_host_texel_wrap states the same two branches on the host):
for a power-of-two size n the sampler takes i & (n - 1) in place of wrap_coord's i % n made non-negative.  The two are the same number for
every int i, in two's complement: checked here for every n = 1, 2, 4 .. 4096 and every i in [-8192, 8192], INT32_MIN, INT32_MAX and +-2^23
(the ends of the sampler's int path), against the remainder stated a third way (Python's floor modulo on unbounded integers)."""
import numpy as np
import pytest

from glaze_amd import abi

POW2 = [1 << k for k in range(13)]          # 1 .. 4096
OTHER = [3, 5, 7, 9, 12, 1000, 4095, 4097]   # sizes that keep the remainder


def coordinates():
    i = np.concatenate([np.arange(-8192, 8193, dtype=np.int64), [-2 ** 31, 2 ** 31 - 1, -2 ** 23, 2 ** 23, -2 ** 23 + 1, 2 ** 23 - 1]])
    return i.astype(np.int32)


def host_wrap(i, n):
    out = np.zeros(len(i), np.int32)
    abi.check(abi.lib().glz_host_texel_wrap(i.ctypes.data, len(i), n, out.ctypes.data))
    return out


@pytest.mark.parametrize("n", POW2 + OTHER)
def test_wrap_is_the_non_negative_remainder(n):
    i = coordinates()
    want = np.array([int(x) % n for x in i], np.int32)            # floor modulo: in [0, n)
    assert np.array_equal(host_wrap(i, n), want)
    # wrap_coord's own rule, C's truncating remainder made non-negative, spelt out
    r = np.fmod(i.astype(np.int64), n)
    assert np.array_equal(np.where(r < 0, r + n, r).astype(np.int32), want)
    if n in POW2:
        assert np.array_equal(i & np.int32(n - 1), want)          # the identity itself, on int32


def test_wrap_rejects_what_no_texture_has():
    i = coordinates()
    out = np.zeros(len(i), np.int32)
    assert abi.lib().glz_host_texel_wrap(i.ctypes.data, len(i), 0, out.ctypes.data) == abi.E_ARG
    assert abi.lib().glz_host_texel_wrap(None, 4, 8, out.ctypes.data) == abi.E_ARG
    assert abi.lib().glz_host_texel_wrap(None, 0, 8, None) == abi.OK
