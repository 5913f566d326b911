"""The per-row table of the sky (glz_host_sky_row_pairs, what scene creation uploads as DeviceScene::sky_rows) is an exact re-arrangement
of its two source arrays: pair y = (marginal value y, conditional integral y), the same 32-bit words, NaN payloads and signed zeros
included.  No device."""
import numpy as np
import pytest

from glaze_amd import abi


def pairs(values, integrals):
    out = np.full(2 * len(values), np.float32(-7.0))
    abi.check(abi.lib().glz_host_sky_row_pairs(values.ctypes.data, integrals.ctypes.data, len(values), out.ctypes.data))
    return out


@pytest.mark.parametrize("n", (1, 2, 7, 32, 1087))
def test_pairs_are_the_source_words_interleaved(n):
    rng = np.random.default_rng(n)
    words = rng.integers(0, 2 ** 32, (2, n), dtype=np.uint64).astype(np.uint32)     # any bit pattern: NaNs, denormals, infinities
    words[0, 0], words[1, -1] = 0x80000000, 0x7FC00123                              # -0.0, a NaN with a payload
    values, integrals = words[0].view(np.float32).copy(), words[1].view(np.float32).copy()
    out = pairs(values, integrals).view(np.uint32)
    assert np.array_equal(out[0::2], words[0]) and np.array_equal(out[1::2], words[1])


def test_no_rows_and_null_arrays():
    assert abi.lib().glz_host_sky_row_pairs(None, None, 0, None) == abi.OK
    a = np.zeros(4, np.float32)
    assert abi.lib().glz_host_sky_row_pairs(None, a.ctypes.data, 4, a.ctypes.data) == abi.E_ARG
    assert abi.lib().glz_host_sky_row_pairs(a.ctypes.data, a.ctypes.data, 4, None) == abi.E_ARG
