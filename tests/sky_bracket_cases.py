"""What tests/test_sky_bracket_host.py and tests/test_gpu_sky_bracket.py share: the xi values at which a bracketed row search can go wrong."""
import numpy as np


def search_points(cdf):
    """float32 xi: every cdf value with its two float neighbours, 0, the float below 1, 1, -0.5 and NaN"""
    cdf = np.asarray(cdf, np.float32)
    up, down = np.nextafter(cdf, np.float32(np.inf)), np.nextafter(cdf, np.float32(-np.inf))
    one = np.float32(1.0)
    ends = np.array([0.0, np.nextafter(one, np.float32(0.0)), 1.0, -0.5, np.nan], np.float32)
    return np.concatenate([cdf, up, down, ends]).astype(np.float32)
