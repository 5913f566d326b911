"""The bracket table of the sky's row search (shading_tables.cpp sky_bracket_table, through glz_host_sky_bracket_table) and the search
that starts inside a bracket (glz_host_sky_cdf_search, the host's statement of device/shading.h sample_cdf).

In a monotone cdf the index the bisection ends on does not depend on the path it takes, so the bracketed search must return the full
search's row and the full search's sample, as float bits -- on cdfs of 2, 3, 17, 1 025 and 1 200 entries with plateaus (rows of weight
zero) and with nothing but zeros, at every cdf value and its two float neighbours, 0, the float below 1, 1, -0.5 and NaN.  A cdf with a
descent (there the path matters) gets the fall-back table, with which every search is the full one."""
import numpy as np
import pytest

from glaze_amd import abi

from sky_bracket_cases import search_points

BUCKETS = 256
FALLBACK = 0xFFFF
SIZES = (2, 3, 17, 1025, 1200)


def monotone_cdf(size, seed, kind):
    """size entries from 0 up: `plateaus` = rows of weight zero in runs (the first and the last row among them), `zeros` = all zero"""
    if kind == "zeros":
        return np.zeros(size, np.float32)
    rng = np.random.default_rng(seed)
    w = rng.random(size - 1) ** 4                       # a few heavy rows: most buckets narrow, some wide
    if kind == "plateaus":
        w[rng.random(size - 1) < 0.4] = 0.0
        w[0] = w[-1] = 0.0
        if size > 3:
            w[size // 2] = 1.0
    total = w.sum()
    c = np.concatenate([[0.0], np.cumsum(w) / (total if total > 0 else 1.0)]).astype(np.float32)
    assert (np.diff(c) >= 0).all()
    return c


def table_of(cdf):
    t = np.zeros(BUCKETS + 1, np.uint16)
    abi.check(abi.lib().glz_host_sky_bracket_table(cdf.ctypes.data, len(cdf), t.ctypes.data))
    return t


def search(cdf, xi, table=None):
    sample, row = np.zeros(len(xi), np.float32), np.zeros(len(xi), np.uint32)
    abi.check(abi.lib().glz_host_sky_cdf_search(cdf.ctypes.data, len(cdf), None if table is None else table.ctypes.data, xi.ctypes.data, len(xi),
                                                sample.ctypes.data, row.ctypes.data))
    return sample, row


@pytest.mark.parametrize("kind", ("plain", "plateaus", "zeros"))
@pytest.mark.parametrize("size", SIZES)
def test_bracketed_search_is_the_full_search(size, kind):
    cdf = monotone_cdf(size, 100 + size, kind)
    table = table_of(cdf)
    # the table: the upper bound of b / 256, stated by numpy
    assert np.array_equal(table, np.searchsorted(cdf, np.arange(BUCKETS + 1, dtype=np.float32) / np.float32(BUCKETS), side="right"))
    xi = np.concatenate([search_points(cdf), np.random.default_rng(size).random(2000, dtype=np.float32)])
    full_s, full_r = search(cdf, xi)
    got_s, got_r = search(cdf, xi, table)
    assert np.array_equal(got_r, full_r)
    assert np.array_equal(got_s.view(np.uint32), full_s.view(np.uint32))
    # and the full search's row is the one a sorted search names: the last entry at or below xi, kept inside [0, size - 2]
    ok = ~np.isnan(xi)
    want = np.clip(np.searchsorted(cdf, xi[ok], side="right").astype(np.int64) - 1, 0, size - 2)
    assert np.array_equal(full_r[ok], want.astype(np.uint32))
    assert (full_r[~ok] == 0).all()


@pytest.mark.parametrize("size", SIZES[1:])
def test_a_descent_gives_the_fall_back_table(size):
    cdf = monotone_cdf(size, 7, "plain")
    k = size // 2
    cdf[k] = np.nextafter(cdf[k - 1], np.float32(-1.0))        # one descent, of one float
    table = table_of(cdf)
    assert (table == FALLBACK).all()
    xi = search_points(cdf)
    full_s, full_r = search(cdf, xi)
    got_s, got_r = search(cdf, xi, table)
    assert np.array_equal(got_r, full_r) and np.array_equal(got_s.view(np.uint32), full_s.view(np.uint32))


def test_fall_back_for_nan_entries_and_for_cdfs_past_16_bits():
    cdf = monotone_cdf(17, 3, "plain")
    cdf[5] = np.nan
    assert (table_of(cdf) == FALLBACK).all()
    assert (table_of(np.linspace(0, 1, 65535, dtype=np.float32)) == FALLBACK).all()
    assert table_of(np.linspace(0, 1, 65534, dtype=np.float32))[BUCKETS] == 65534


def test_arguments():
    cdf = monotone_cdf(17, 3, "plain")
    xi, s, r = np.zeros(4, np.float32), np.zeros(4, np.float32), np.zeros(4, np.uint32)
    L = abi.lib()
    assert L.glz_host_sky_bracket_table(cdf.ctypes.data, 17, None) == abi.E_ARG
    assert L.glz_host_sky_cdf_search(cdf.ctypes.data, 1, None, xi.ctypes.data, 4, s.ctypes.data, r.ctypes.data) == abi.E_ARG
    assert L.glz_host_sky_cdf_search(cdf.ctypes.data, 17, None, None, 4, s.ctypes.data, r.ctypes.data) == abi.E_ARG
    foreign = table_of(monotone_cdf(1025, 3, "plain"))      # a table of a longer cdf would walk the search past this one's end
    assert L.glz_host_sky_cdf_search(cdf.ctypes.data, 17, foreign.ctypes.data, xi.ctypes.data, 4, s.ctypes.data, r.ctypes.data) == abi.E_ARG
