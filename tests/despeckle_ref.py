"""What the firefly-rejection tests share: a float64 numpy restatement of the rule as the header comment of glz_despeckle_params
(include/glaze_abi.h) specifies it -- written from that comment, not from the C++ -- and the planting of outliers into the synthetic
frames of denoise_ref.py."""
import numpy as np

from denoise_ref import DEFAULTS as DENOISE_DEFAULTS, _shift, synthetic_frame

DEFAULTS = dict(radius=2, trim=2, ratio=8.0)


def reference_despeckle(result, aov0, aov1, eps_albedo=DENOISE_DEFAULTS["eps_albedo"], **params):
    """float64 restatement of the specification; inputs are taken as they are (float32 values).  Returns
    out (H x W x 4 float64: i_0' x A, .w passed through), clamped (H x W bool), L / T per pixel (NaN where p is no candidate, m <= trim or T
    is not >= 0) and the smallest |L(p) / T - 1| over the candidates that have a threshold."""
    P = dict(DEFAULTS, **params)
    R, trim, ratio = int(P["radius"]), int(P["trim"]), float(np.float32(P["ratio"]))
    with np.errstate(all="ignore"):
        c = result[..., :3].astype(np.float64)
        z = aov0[..., 3].astype(np.float64)
        a = aov1[..., :3].astype(np.float64)
        eps_a = float(np.float32(eps_albedo))
        A = np.where(a > eps_a, a, eps_a)
        i0 = c / A
        L = (i0[..., 0] + i0[..., 1]) + i0[..., 2]
        usable = np.isfinite(z) & np.isfinite(i0).all(-1)
        Ls, us = [], []
        for dy in range(-R, R + 1):
            for dx in range(-R, R + 1):
                if dx == 0 and dy == 0:
                    continue
                us.append(_shift(usable, dy, dx, False))
                Ls.append(np.where(us[-1], _shift(L, dy, dx, 0.0), -np.inf))
        Ls, us = np.stack(Ls, -1), np.stack(us, -1)
        m = us.sum(-1)
        M = -np.sort(-Ls, axis=-1)[..., trim]                     # the (trim + 1)-th largest with multiplicity (-inf entries sort last)
        mu = np.where(us, np.minimum(Ls, M[..., None]), 0.0).sum(-1) / np.maximum(m, 1)
        T = ratio * mu
        has_T = usable & (m > trim) & (T >= 0)
        clamped = has_T & (L > T)
        f = np.where(clamped, T / np.where(clamped, L, 1.0), 1.0)
        out = np.concatenate([np.where(clamped[..., None], i0 * f[..., None], i0) * A, result[..., 3:4].astype(np.float64)], -1)
        over = np.where(has_T, L / T, np.nan)
        near = np.abs(over - 1.0)
        nearest = np.nanmin(near) if np.isfinite(near).any() else np.inf
    return out, clamped, over, nearest


def plant_outliers(result, region, seed, n=40, with_non_finite=False):
    """Multiplies n hit pixels (drawn without replacement from a seeded generator, none adjacent to another, at least 3 pixels from the frame's and
    the regions' borders where the frame allows) by 50, 1e3 and 1e5 in turn, the last of them together with its right-hand neighbour: one
    adjacent pair.  with_non_finite: also a NaN, a +inf and a -inf pixel (one channel each) on three further hit pixels.
    Returns the planted frame and the (y, x) lists of the outliers and of the non-finite pixels."""
    rng = np.random.default_rng(seed)
    h, w = region.shape
    out = result.copy()
    ys, xs = np.nonzero(region > 0)
    order = rng.permutation(len(ys))
    taken = np.zeros((h, w), bool)
    spots = []
    want = n - 1 + (3 if with_non_finite else 0)
    for j in order:
        y, x = int(ys[j]), int(xs[j])
        if x + 2 >= w or taken[max(0, y - 3):y + 4, max(0, x - 3):x + 5].any() or region[y, x + 1] == 0:
            continue
        taken[y, x] = True
        spots.append((y, x))
        if len(spots) == want:
            break
    assert len(spots) == want, "the frame is too small for the outliers"
    bad = spots[n - 1:]
    spots = spots[:n - 1]
    factors = (50.0, 1e3, 1e5)
    for k, (y, x) in enumerate(spots):
        out[y, x, :3] *= np.float32(factors[k % 3])
    y, x = spots[-1]
    out[y, x + 1, :3] *= np.float32(factors[(len(spots) - 1) % 3])      # the adjacent pair
    spots = spots + [(y, x + 1)]
    for (y, x), v, ch in zip(bad, (np.nan, np.inf, -np.inf), (1, 0, 2)):
        out[y, x, ch] = v
    return out, spots, bad


_FRAMES = {}


def planted_frame(width, height, spp, seed, with_non_finite=True):
    """synthetic_frame with 40 planted outliers (and the three non-finite pixels), made once and shared read-only:
    result, planted, aov0, aov1, region, outliers, non-finite pixels"""
    key = (width, height, spp, seed, with_non_finite)
    if key not in _FRAMES:
        result, aov0, aov1, region = synthetic_frame(width, height, seed, spp=spp)
        planted, spots, bad = plant_outliers(result, region, seed, n=40, with_non_finite=with_non_finite)
        for a in (result, planted, aov0, aov1, region):
            a.setflags(write=False)
        _FRAMES[key] = (result, planted, aov0, aov1, region, spots, bad)
    return _FRAMES[key]
