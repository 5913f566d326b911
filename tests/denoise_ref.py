"""What the denoiser tests share: seeded synthetic frames and a float64 numpy restatement of the filter as the header comment of
glz_denoise_params (include/glaze_abi.h) specifies it -- written from that comment, not from the C++."""
import numpy as np

DEFAULTS = dict(iterations=5, sigma_color=4.0, sigma_depth=1.0, normal_power_log2=6, eps_albedo=1.0 / 256.0, eps_depth=1e-3, eps_color=1e-8)
MISS = np.uint32(0xFFFFFFFF)


def synthetic_frame(width, height, seed, spp=4, irradiance=None):
    """Two planes and a sky strip: rows < H/5 are misses, below them a wall (normal +z) down to H/2, then a floor (normal +y, perpendicular
    to the wall's).  Checkerboard albedo, depth planar per region, colour = irradiance x gamma noise (spp-sample mean) x albedo, float32.
    irradiance: None = smooth in x and y, or a constant.  Returns result, aov0, aov1 (H x W x 4 float32) and the region map (0 sky, 1 wall, 2 floor)."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:height, 0:width]
    region = np.where(y < height // 5, 0, np.where(y < height // 2, 1, 2))
    hit = region > 0
    normal = np.zeros((height, width, 3), np.float32)
    normal[region == 1] = (0.0, 0.0, 1.0)
    normal[region == 2] = (0.0, 1.0, 0.0)
    depth = np.where(region == 1, 6.0 + 0.01 * x, 6.0 + 0.004 * x - 0.03 * (y - height // 2)).astype(np.float32)
    depth[~hit] = np.inf
    check = ((x // 8 + y // 8) % 2).astype(np.float32)
    albedo = np.stack([0.15 + 0.7 * check, 0.2 + 0.5 * check, 0.8 - 0.6 * check], -1).astype(np.float32)
    albedo[~hit] = 1.0
    if irradiance is None:
        e = 1.0 + 0.5 * np.sin(x / 23.0) * np.cos(y / 17.0)
        e = np.where(hit, e, 0.6 + 0.3 * x / width)
        noise = rng.gamma(spp, 1.0 / spp, size=(height, width, 3))
    else:
        e = np.full((height, width), float(irradiance))
        noise = np.ones((height, width, 3))
    colour = (np.float32(1.0) * (e[..., None] * noise).astype(np.float32)) * albedo
    result = np.concatenate([colour.astype(np.float32), np.ones((height, width, 1), np.float32)], -1)
    result[..., 3] = rng.integers(0, 2, size=(height, width)).astype(np.float32)      # .w only passes through: make it recognisable
    inst = np.where(hit, region - 1, MISS).astype(np.uint32)
    aov0 = np.concatenate([normal, depth[..., None]], -1).astype(np.float32)
    aov1 = np.concatenate([albedo, inst.view(np.float32)[..., None]], -1).astype(np.float32)
    return np.ascontiguousarray(result), np.ascontiguousarray(aov0), np.ascontiguousarray(aov1), region


def _shift(a, dy, dx, fill):
    """a[y + dy, x + dx] with `fill` outside the image"""
    h, w = a.shape[:2]
    out = np.full_like(a, fill)
    ys, yd = (slice(dy, h), slice(0, h - dy)) if dy >= 0 else (slice(0, h + dy), slice(-dy, h))
    xs, xd = (slice(dx, w), slice(0, w - dx)) if dx >= 0 else (slice(0, w + dx), slice(-dx, w))
    if abs(dy) < h and abs(dx) < w:
        out[yd, xd] = a[ys, xs]
    return out


def _slope(z, axis):
    f = _shift(z, 1 if axis == 0 else 0, 1 if axis == 1 else 0, np.nan) - z          # z(next) - z(p); NaN where there is no next
    b = z - _shift(z, -1 if axis == 0 else 0, -1 if axis == 1 else 0, np.nan)
    okf, okb = np.isfinite(f), np.isfinite(b)
    return np.where(okf & okb, np.where(np.abs(b) < np.abs(f), b, f), np.where(okf, f, np.where(okb, b, 0.0)))


def reference_denoise(result, aov0, aov1, **params):
    """float64 restatement of the specification; inputs are taken as they are (float32 values), the output is float64"""
    P = dict(DEFAULTS, **params)
    with np.errstate(all="ignore"):
        c = result[..., :3].astype(np.float64)
        n = aov0[..., :3].astype(np.float64)
        z = aov0[..., 3].astype(np.float64)
        a = aov1[..., :3].astype(np.float64)
        eps_a = float(np.float32(P["eps_albedo"]))
        A = np.where(a > eps_a, a, eps_a)
        i = c / A
        hit = np.isfinite(z)
        gx, gy = _slope(z, 1), _slope(z, 0)
        h5 = (1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16)
        sd, ez, ec = (float(np.float32(P[k])) for k in ("sigma_depth", "eps_depth", "eps_color"))
        for k in range(P["iterations"]):
            s = 2 ** k
            S = (float(np.float32(P["sigma_color"])) / s) ** 2
            fin_p = np.isfinite(i).all(-1)
            Pv = np.where(fin_p[..., None], i, 0.0)
            NP = (Pv * Pv).sum(-1)
            sw = np.zeros(z.shape)
            acc = np.zeros(i.shape)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    Q = _shift(i, s * dy, s * dx, np.nan)
                    use = np.isfinite(Q).all(-1)
                    if dx == 0 and dy == 0:
                        W = np.ones(z.shape)
                    else:
                        zq = _shift(z, s * dy, s * dx, np.nan)
                        nq = _shift(n, s * dy, s * dx, 0.0)
                        use &= np.isfinite(zq) == hit
                        D = Q - Pv
                        cn = S * ((NP + (Q * Q).sum(-1)) + ec)
                        cd = cn + (D * D).sum(-1)
                        wn = np.maximum((n * nq).sum(-1), 0.0)
                        for _ in range(P["normal_power_log2"]):
                            wn = wn * wn
                        ax, ay = s * dx * gx, s * dy * gy
                        a = (zq - z) - (ax + ay)
                        b = sd * ((np.abs(ax) + np.abs(ay)) + ez * z)
                        W = np.where(hit, (wn * (cn * b * b)) / (cd * (b * b + a * a)), cn / cd)
                        use &= W > 0
                    hw = np.where(use, h5[dy + 2] * h5[dx + 2] * W, 0.0)
                    sw += hw
                    acc += hw[..., None] * np.where(use[..., None], Q, 0.0)
            i = np.where((sw > 0)[..., None], acc / sw[..., None], i)
        out = np.concatenate([i * A, result[..., 3:4].astype(np.float64)], -1)
    return out
