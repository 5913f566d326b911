"""from_surface_color / from_illuminant_color on the device (device/shading.h, through glz_debug_color_to_spec) against the oracle's
orc_dev_from_surface_color / orc_dev_from_illuminant_color, bit for bit.

The arithmetic -- ((white * k0 + A * k1) + B * k2) * scale, no contraction, the basis pair (A, B) by the ordering of r, g, b -- is the
same on both sides, so every bin has to come out with the same bits: for each of the six orderings of (r, g, b), on every tie (the
comparisons are <=, the first branch that holds wins), for zeros, negatives, values above 1, infinities and NaNs."""
import itertools

import numpy as np
import pytest

from oracle import pyoracle

pytestmark = pytest.mark.gpu


def colours():
    rows = []
    for lo, mid, hi in ((0.1, 0.5, 0.9), (0.0, 0.25, 1.0), (-0.75, 0.5, 2.5), (1.5, 3.0, 70000.0), (-3.0, -2.0, -1.0), (1e-40, 1e-39, 1e-38)):
        rows += list(itertools.permutations((lo, mid, hi)))                  # the six orderings
    for a, b in ((0.3, 0.7), (0.7, 0.3), (0.0, 1.0), (1.0, 0.0), (-1.0, 2.0), (2.0, -1.0), (0.0, -0.0), (-0.0, 0.0)):
        rows += [(a, a, b), (a, b, a), (b, a, a)]                            # r = g, r = b, g = b, the pair below and above the third
    rows += [(v, v, v) for v in (0.0, -0.0, 0.5, 1.0, 2.0, -1.0)]            # all equal
    special = (0.0, 0.5, -0.5, 1.5, np.inf, -np.inf, np.nan)
    rows += [c for c in itertools.product(special, repeat=3) if not all(np.isfinite(c))]   # every place an infinity or a NaN can stand
    out = np.array(rows, np.float32)
    payload = np.array([0x7FC00001, 0xFFC00000, 0x7F800001, 0x7FFFFFFF], np.uint32).view(np.float32)   # NaNs other than numpy's
    extra = np.full((payload.size * 3, 3), 0.25, np.float32)
    for k in range(payload.size):
        for ch in range(3):
            extra[3 * k + ch, ch] = payload[k]
    rng = np.random.default_rng(7)
    rand = np.concatenate([rng.random((3000, 3)), rng.uniform(-2.0, 4.0, (1000, 3)), np.round(rng.random((1000, 3)) * 4.0) / 4.0])   # the last: many ties
    return np.concatenate([out, extra, rand.astype(np.float32)])


@pytest.mark.parametrize("illuminant", [False, True], ids=["surface", "illuminant"])
def test_color_to_spectrum_equals_the_oracle_bit_for_bit(instance, illuminant):
    """every word of every bin, the NaNs' signs and payloads included"""
    rgb = colours()
    fn = pyoracle.lib().orc_dev_from_illuminant_color if illuminant else pyoracle.lib().orc_dev_from_surface_color
    want = np.zeros((rgb.shape[0], 16), np.float32)
    for i in range(rgb.shape[0]):
        fn(rgb[i].ctypes.data, want[i].ctypes.data)
    assert np.isfinite(want).all(-1).sum() > 5000 and np.isnan(want).any(-1).sum() > 100 and np.isinf(want).any(-1).sum() > 20   # the inputs reach all three
    got = instance.debug_color_to_spec(rgb, illuminant)
    diff = got.view(np.uint32) != want.view(np.uint32)
    print("%d colours, %d with a word that differs, %d words differ, %d of them NaN on both sides" % (
        rgb.shape[0], int(diff.any(-1).sum()), int(diff.sum()), int((diff & np.isnan(got) & np.isnan(want)).sum())))
    assert not diff.any(), "first colours that differ: %s" % rgb[diff.any(-1)][:5].tolist()
