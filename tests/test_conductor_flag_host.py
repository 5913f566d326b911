"""The `conductor_finite` flag of a pair of metal spectra (glz_host_conductor_finite: what scene creation and material updates put into
the top bit of MatCompact::spectra).  A flagged pair promises that fresnel_conductor is finite in every bin for every cosine |c| <= 2,
which is what lets an Uber hit with a zero metalness skip the term (its product with the metalness is then a zero).

  * every built-in metal of glz_tables.h with its flag: the list below records which pairs have it.  A pair without it is no error -- its
    materials run the unshortened code -- but a change of the list is a change of the rule and has to be looked at;
  * pairs that must not get it: all-zero spectra (the first denominator is c^2), k = 0 with n <= 2 (a = n^2: the denominator (n + c)^2
    reaches 0 inside the range), a NaN or an infinity in a single bin, |a| > 2^60;
  * the promise itself: for every flagged built-in pair, fresnel_conductor in float32 -- the device routine's operations in their order,
    each one rounded to float32 as numpy does -- at 10 001 cosines evenly spaced over [-2, 2] and at +0 and -0 is finite in every bin.
"""
import ctypes as C

import numpy as np

from glaze_amd import abi

METALS = ("SILVER", "ALUMINIUM", "GOLD", "COPPER", "IRON", "MERCURY", "LEAD", "PLATINUM", "TUNGSTEN", "BERYLLIUM", "BISMUTH", "COBALT",
          "CHROMIUM", "GERMANIUM", "POTASSIUM", "LITHIUM", "MAGNESIUM", "MANGANESE", "MOLYBDENUM", "SODIUM", "NIOBIUM", "NICKEL", "PALLADIUM",
          "RHODIUM", "TANTALUM", "TITANIUM", "VANADIUM", "ZINC", "ZIRCONIUM")
# Germanium's k falls to 0.38 at n = 4.97 in the red bins: the second denominator's minimum k^2 / a = 0.006 at c = -n / a = -0.2 is below
# 2^-10 (a + 4 n + 5) = 0.048.  (The float quotient there is finite all the same; the rule does not try to know that.)
UNFLAGGED = ("GERMANIUM",)


def flag(n, a):
    n, a = np.ascontiguousarray(n, np.float32), np.ascontiguousarray(a, np.float32)
    assert n.shape == a.shape == (16,)
    out = C.c_int(-1)
    abi.check(abi.lib().glz_host_conductor_finite(n.ctypes.data, a.ctypes.data, C.byref(out)))
    assert out.value in (0, 1)
    return bool(out.value)


def metal(index):
    n, a = np.zeros(16, np.float32), np.zeros(16, np.float32)
    abi.check(abi.lib().glz_host_metal_spectra(index, n.ctypes.data, a.ctypes.data))
    return n, a


def fresnel_conductor_f32(c, n, a):
    """device/shading.h's fresnel_conductor: c (m,) float32, n / a (16,) float32 -> (m, 16) float32, every operation in float32"""
    c = np.asarray(c, np.float32)[:, None]
    one, two = np.float32(1.0), np.float32(2.0)
    with np.errstate(all="ignore"):
        c2, twoc = c * c, c * two
        e = n[None, :] * twoc
        ep, epp = e + c2, e + one
        perp = (a - ep) / (a + ep)
        tmp = a * c2
        par = (tmp - epp) / (tmp + epp)
        r = (perp + par) / two
    assert r.dtype == np.float32
    return r


def test_built_in_metals_and_their_flags():
    assert len(METALS) == 29
    assert abi.lib().glz_host_metal_spectra(len(METALS), metal(0)[0].ctypes.data, metal(0)[1].ctypes.data) == abi.E_ARG
    got = {name: flag(*metal(i)) for i, name in enumerate(METALS)}
    print("pairs without the flag: %s" % sorted(k for k, v in got.items() if not v))
    assert got == {name: name not in UNFLAGGED for name in METALS}
    # the pair is what a material record carries: n, and n^2 + k^2 in float32
    n, a = metal(2)
    assert n[0] == np.float32(1.46212888) and a[0] == np.float32(1.46212888) * np.float32(1.46212888) + np.float32(1.9556787) * np.float32(1.9556787)


def test_pairs_that_must_not_be_flagged():
    zero = np.zeros(16, np.float32)
    assert not flag(zero, zero)                                               # a = 0, n = 0: the denominator is c^2
    for n in (0.05, 0.5, 1.0, 1.5, 2.0):                                      # k = 0, n <= 2: a = n^2, (n + c)^2 = 0 at c = -n
        nn = np.full(16, n, np.float32)
        assert not flag(nn, nn * nn), n
    good_n, good_a = metal(0)
    assert flag(good_n, good_a)
    for bad in (np.nan, np.inf, -np.inf):                                     # a single bin, in either spectrum
        for which in (0, 1):
            for b in (0, 7, 15):
                pair = [good_n.copy(), good_a.copy()]
                pair[which][b] = bad
                assert not flag(*pair), (bad, which, b)
    for b in (0, 15):                                                          # |a| > 2^60, |n| > 2^60
        a = good_a.copy()
        a[b] = np.nextafter(np.float32(2.0 ** 60), np.float32(np.inf))
        assert not flag(good_n, a)
        a[b] = -a[b]
        assert not flag(good_n, a)
        n = good_n.copy()
        n[b] = np.nextafter(np.float32(2.0 ** 60), np.float32(np.inf))
        assert not flag(n, good_a)
    # one bad bin is enough, and it need not be the first: silver with bin 9 of the all-zero pair
    n, a = good_n.copy(), good_a.copy()
    n[9] = a[9] = 0.0
    assert not flag(n, a)
    null = abi.lib().glz_host_conductor_finite(None, good_a.ctypes.data, C.byref(C.c_int()))
    assert null == abi.E_ARG


def test_flagged_built_in_pairs_are_finite_in_float32_over_the_whole_range():
    c = np.concatenate([np.linspace(-2.0, 2.0, 10001).astype(np.float32), np.array([0.0, -0.0], np.float32)])
    assert c[0] == -2 and c[10000] == 2 and np.signbit(c[-1]) and not np.signbit(c[-2])
    checked = 0
    for i, name in enumerate(METALS):
        n, a = metal(i)
        if not flag(n, a):
            continue
        r = fresnel_conductor_f32(c, n, a)
        assert r.shape == (10003, 16) and np.isfinite(r).all(), name
        assert np.abs(r).max() < 2.0 ** 12, name                              # the bound the rule's margin gives the quotients
        checked += 1
    assert checked == len(METALS) - len(UNFLAGGED)
    # and the rule is no formality: the all-zero pair it refuses is NaN at c = 0 (0 / 0)
    zero = np.zeros(16, np.float32)
    assert np.isnan(fresnel_conductor_f32(np.array([0.0], np.float32), zero, zero)).all()
