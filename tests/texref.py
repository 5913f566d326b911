"""A float64 reference of the texture sampler (device/shading.h bilinear_level / texture2d_lod, oracle.cpp texture_bilinear_level /
texture_lod), written from the rules alone: it shares no code and no table with either side.

The rules: texel centres at (i + 0.5) / size, bilinear weights, REPEAT wrap (exact, for every coordinate), formats GRAY (g, 0, 0, 1),
RGBA_NORM (c / 255) and RGBA_SRGB (the sRGB EOTF of c / 255 for r, g, b; a / 255), LINEAR blending of the two nearest mip levels of
the level lam = lod_base + 0.5 log2(w h) clamped to [0, levels - 1], and `taps` probes spread over (du, dv) and averaged.

Where the sampler's position comes from is part of the rule, not of its arithmetic: the sample point is the float32 value u * w - 0.5
(two IEEE operations), and a probe sits at the float32 value u + ((k + 0.5) / taps - 0.5) * du.  Those few operations are done in
float32 here too; everything after them -- floor, wrap, weights, decode, blends, average -- is float64 and exact or nearly so.
"""
import numpy as np

U = 2.0 ** -24          # unit roundoff of float32


def eotf(c):
    c = np.asarray(c, np.float64)
    return np.where(c <= 0.04045, c / 12.92, ((c + 0.055) / 1.055) ** 2.4)


def decode(fmt, px):
    """texels (h, w, 4) float64 of a level stored as (h, w) gray or (h, w, 4) RGBA8"""
    from glaze_amd import abi
    px = np.asarray(px)
    if fmt == abi.TEX_GRAY:
        g = px.astype(np.float64) / 255.0
        return np.stack([g, np.zeros_like(g), np.zeros_like(g), np.ones_like(g)], -1)
    t = px.astype(np.float64) / 255.0
    if fmt == abi.TEX_RGBA_SRGB:
        t[..., :3] = eotf(t[..., :3])
    return t


def sample_point(u, size):
    """the float32 sample point u * size - 0.5"""
    with np.errstate(over="ignore", invalid="ignore"):
        return (np.asarray(u, np.float32) * np.float32(size) - np.float32(0.5)).astype(np.float64)


def wrap_index(f, n):
    """floor(f) mod n, exact for every finite f (float64 holds any float32 exactly; np.fmod is exact); non-finite -> 0"""
    fl = np.floor(np.where(np.isfinite(f), f, 0.0))
    r = np.fmod(fl, n)
    return np.where(r < 0, r + n, r).astype(np.int64), f - fl


def bilinear(tex, u, v):
    """(value (n, 4), lo (n, 4), hi (n, 4)) of a bilinear fetch: lo / hi = min / max of the four texels blended"""
    h, w = tex.shape[:2]
    fu, fv = sample_point(u, w), sample_point(v, h)
    x0, ax = wrap_index(fu, w)
    y0, ay = wrap_index(fv, h)
    x1, y1 = (x0 + 1) % w, (y0 + 1) % h
    a, b, c, d = tex[y0, x0], tex[y0, x1], tex[y1, x0], tex[y1, x1]
    ax, ay = ax[:, None], ay[:, None]
    with np.errstate(invalid="ignore"):
        val = (a * (1 - ax) + b * ax) * (1 - ay) + (c * (1 - ax) + d * ax) * ay
    lo = np.minimum(np.minimum(a, b), np.minimum(c, d))
    hi = np.maximum(np.maximum(a, b), np.maximum(c, d))
    bad = ~(np.isfinite(fu) & np.isfinite(fv))
    val[bad] = np.nan
    return val, lo, hi


def ulp32(x):
    return np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)


def level0_bound(val, lo, hi, u, size_u, v, size_v):
    """per-channel error bound of a float32 fetch: (max - min) * 2 ulp32(|u w| + 1) + 4 * 2^-24 * max|texel|.  The lerps' roundings
    are at most 2 u |b - a| + u |result| each (three of them per channel, texels >= 0), the decode adds u |texel|; the sample point and
    the weights ax = fu - floor(fu) are exact in float32, so no term for them is needed -- the first term is the lerps' share."""
    with np.errstate(over="ignore", invalid="ignore"):
        s = np.maximum(np.abs(np.asarray(u, np.float64) * size_u), np.abs(np.asarray(v, np.float64) * size_v)) + 1.0
    s = np.where(np.isfinite(s), np.minimum(s, 3.0e38), 3.0e38)
    return (hi - lo) * 2 * ulp32(s)[:, None] + 4 * U * np.abs(hi)


def lod(levels, u, v, lod_base, du, dv, taps):
    """texture2d_lod's rule on the decoded levels (list of (h, w, 4) float64): (value (n, 4), bound (n, 4)).  All arguments are
    arrays of n (taps as integers 1..16)."""
    n = len(u)
    u, v = np.asarray(u, np.float32), np.asarray(v, np.float32)
    lod_base = np.asarray(lod_base, np.float32)
    du, dv, taps = np.asarray(du, np.float32), np.asarray(dv, np.float32), np.asarray(taps, np.int64)
    h0, w0 = levels[0].shape[:2]
    top = len(levels) - 1
    use = (lod_base > np.float32(-1e29)) & (top > 0)
    with np.errstate(invalid="ignore"):
        lam = lod_base.astype(np.float64) + 0.5 * np.log2(float(w0) * float(h0))
    lam = np.where(lam > 0, lam, 0.0)             # NaN -> 0
    lam = np.minimum(lam, top)
    lam = np.where(use, lam, 0.0)
    probes = np.where(use, taps, 1)
    l0 = np.floor(lam).astype(np.int64)
    frac = lam - l0
    # the level's float32 arithmetic (glz_log2f within a few ulp, one add, one multiply): |d lam| <= 8 ulp32(|lam| + |lod_base| + 1).
    # The blend is continuous in lam, so that moves the result by at most |d lam| times a texel difference (texels lie in [0, 1]).
    dlam = np.where(use & (lam > 0) & (lam < top), 8 * ulp32(np.abs(lam) + np.abs(lod_base.astype(np.float64)) + 1.0), 0.0)
    out = np.zeros((n, 4))
    bound = np.zeros((n, 4))
    mag = np.zeros((n, 4))
    for k in range(16):
        live = k < probes
        if not live.any():
            break
        with np.errstate(over="ignore", invalid="ignore"):
            s = (np.float32(k) + np.float32(0.5)) / probes.astype(np.float32) - np.float32(0.5)
            uu = np.where(probes > 1, u + s * du, u).astype(np.float32)
            vv = np.where(probes > 1, v + s * dv, v).astype(np.float32)
        val = np.full((n, 4), np.nan)
        b = np.zeros((n, 4))
        lo_p, hi_p = np.full((n, 4), np.inf), np.full((n, 4), -np.inf)
        for l in np.unique(l0[live]):
            for upper in (0, 1):
                sel = live & (l0 == l) & ((frac > 0) if upper else True)
                if not sel.any() or l + upper > top:
                    continue
                tex = levels[l + upper]
                h, w = tex.shape[:2]
                vl, lo, hi = bilinear(tex, uu[sel], vv[sel])
                bl = level0_bound(vl, lo, hi, uu[sel], w, vv[sel], h)
                f = frac[sel][:, None] if upper else 1.0 - frac[sel][:, None]
                if upper:
                    val[sel] = val[sel] + f * vl
                    b[sel] += bl
                else:
                    val[sel] = f * vl
                    b[sel] = bl
                lo_p[sel] = np.minimum(lo_p[sel], lo)
                hi_p[sel] = np.maximum(hi_p[sel], hi)
        two = live & (frac > 0)
        # the level blend's own lerp: 2 u |b - a| + u |result|
        b[two] += 2 * U * (hi_p[two] - lo_p[two]) + U * np.abs(hi_p[two])
        out[live] += val[live]
        bound[live] += b[live]
        mag[live] = np.maximum(mag[live], np.abs(hi_p[live]))
    pr = probes[:, None].astype(np.float64)
    out /= pr
    bound = bound / pr + (pr + 1) * U * mag + dlam[:, None]
    return out, bound
