"""What the motion / reprojection tests share: a float64 numpy restatement of the specification in the header comment above
glz_reproject_params (include/glaze_abi.h) -- written from that comment, not from the C++ -- and seeded inputs for it."""
import numpy as np

from glaze_amd.scene_desc import make_camera

from denoise_ref import MISS, _slope, synthetic_frame

EPS = 2.0 ** -24
DEFAULT_TOLERANCE = 1.0 / 64.0


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------------
# project_point
# ---------------------------------------------------------------------------------------------------------------------
def reference_project(world2camera, camera2screen, persp, w, h, points):
    """float64 project_point on the ROUNDED matrices (16 float32 each, column-major).  Returns (fx, fy, z) with (0, 0, inf) where invalid,
    the valid mask, and the camera-space depth z_c (-Pc.z) the error bound divides by."""
    M = np.asarray(world2camera, np.float64).reshape(4, 4).T
    S = np.asarray(camera2screen, np.float64).reshape(4, 4).T
    P = np.asarray(points, np.float64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        Pc = P @ M[:3, :3].T + M[:3, 3]
        d = -Pc[:, 2]
        if persp:
            ndc = (Pc @ S[:2, :3].T + S[:2, 3]) / d[:, None]
            z = np.sqrt((Pc * Pc).sum(-1))
            front = d > 0
        else:
            ndc = Pc[:, :2]
            z = d
            front = np.ones(len(P), bool)
        fx, fy = (ndc[:, 0] + 1.0) * 0.5 * w, (ndc[:, 1] + 1.0) * 0.5 * h
        # finite() of the specification is a binary32 notion: |v| <= FLT_MAX
        fmax = float(np.finfo(np.float32).max)
        valid = front & (np.abs(z) <= fmax) & (z > 0) & (np.abs(fx) <= fmax) & (np.abs(fy) <= fmax)
        # ... and so is every operation: an intermediate beyond FLT_MAX is an infinity there, which reaches z, fx or fy in every case
        valid &= (np.abs(P[:, None, :] * M[None, :3, :3]).max((1, 2)) <= fmax) & (np.abs(Pc).max(-1) <= fmax) & (((Pc * Pc).sum(-1) <= fmax) | (not persp))
        valid &= np.abs(ndc).max(-1) <= fmax
    out = np.stack([np.where(valid, fx, 0.0), np.where(valid, fy, 0.0), np.where(valid, z, np.inf)], -1)
    return out, valid, d


def projection_bounds(camera2screen, persp, w, h, points, eye, z_c, z):
    """The issue's bound per point: 32 * 2^-24 * F * S / z_c for fx and fy (F = (W/2)|p0|, (H/2)|p5|), and the same with F = 1 as a RELATIVE
    bound on the depth.  About 23 rounded operations and the matrices' own rounding lie between the inputs and a coordinate, each at most
    2^-24 * S with S = |P'|_1 + |eye|_1; 32 is that count rounded up to a power of two.  An orthographic camera has no perspective
    division: p0 = p5 = 1 and z_c = 1 for fx and fy there, and the depth is relative to itself."""
    S = np.abs(np.asarray(points, np.float64)).sum(-1) + np.abs(np.asarray(eye, np.float64)).sum()
    p0, p5 = (abs(float(camera2screen[0])), abs(float(camera2screen[5]))) if persp else (1.0, 1.0)
    zc = z_c if persp else np.ones_like(z_c)
    k = 32.0 * EPS * S
    return k * (w / 2.0) * p0 / zc, k * (h / 2.0) * p5 / zc, k / (z_c if persp else z)


# ---------------------------------------------------------------------------------------------------------------------
# inputs of the projection tests (host against float64, device against host)
# ---------------------------------------------------------------------------------------------------------------------
FOV = np.float32(np.radians(np.float32(70.0)))


def cameras():
    """name -> camera: per type one whose matrices are exact in binary32 (integer eye, axis-aligned view: the points on and beside the
    eye then take the same side in binary32 and binary64) and one in general position"""
    return {
        "perspective, axis-aligned": make_camera(position=(2, 1, -4), target=(2, 1, 10), fovx=np.float32(np.pi / 2), near=1e-2, far=100.0),
        "perspective, general": make_camera(position=(-18, 2.0, -18), target=(10, 1.0, 10), fovx=FOV, near=1e-2, far=200.0),
        "orthographic, axis-aligned": make_camera(position=(2, 1, -4), target=(2, 1, 10), near=1e-2, far=100.0, orthographic=True, scale=3.0),
        "orthographic, general": make_camera(position=(3, 2.5, -6), target=(0.5, 0.25, 1.0), near=1e-2, far=100.0, orthographic=True, scale=2.0),
    }


def projection_points(camera, n, seed):
    """n world points: a cloud around the view axis on both sides of the eye, kept where the decision `in front` is not a matter of
    rounding; with an exact camera also the eye itself, points beside it (in its plane) and straight behind it; NaN, +-inf and 1e30."""
    rng = np.random.default_rng(seed)
    eye, target = np.array(camera.position[:], np.float64), np.array(camera.target[:], np.float64)
    axis = (target - eye) / np.linalg.norm(target - eye)
    pts = eye + rng.uniform(-30, 30, (4 * n, 1)) * axis + rng.normal(0, 6, (4 * n, 3))
    pts = pts.astype(np.float32)
    depth = (pts.astype(np.float64) - eye) @ axis
    pts = pts[np.abs(depth) > 1e-3 * (np.abs(pts).sum(-1) + np.abs(eye).sum())][:n - 16]
    special = [eye, eye + (1, 0, 0), eye + (0, -2, 0), eye - 3 * axis, eye + 5 * axis, eye + (0.5, 0.25, 0) + 2 * axis] if np.allclose(np.abs(axis).max(), 1.0) else []
    odd = [(np.nan, 0, 0), (0, np.nan, 1), (np.inf, 0, 0), (0, -np.inf, 0), (0, 0, np.inf), (1e30, 0, 0), (0, 1e30, 5), (0, 0, -1e30), (1e30, 1e30, 1e30), (-np.inf, np.nan, 0)]
    extra = np.array(special + odd, np.float64).astype(np.float32)
    return np.ascontiguousarray(np.concatenate([extra, pts])[:n])


# size, shift of the reprojection cases (host against float64, device against host)
REPROJECT_CASES = [((150, 83), (3.0, -2.0)), ((150, 83), (-1.5, 0.5)), ((97, 61), (0.0, 0.0)), ((97, 61), (2.25, 4.75))]


# ---------------------------------------------------------------------------------------------------------------------
# the reprojection rule
# ---------------------------------------------------------------------------------------------------------------------
def reference_reproject(motion, color, aov0, aov1, depth_tolerance=DEFAULT_TOLERANCE):
    """float64 restatement; inputs are taken as they are (float32 values).  Returns out (H x W x 4 float64), the accepted taps (H x W x 4
    bool, tap order: dy outer, dx inner) and the pixels that sit on a decision: a tap whose |zh - z'| / z' lies within 1e-4 relative of the
    tolerance, or a q within 1e-4 of an integer."""
    h, w = motion.shape[:2]
    tol = float(np.float32(depth_tolerance))
    m = motion.astype(np.float64)
    c = color[..., :3].astype(np.float64)
    z = aov0[..., 3].astype(np.float64)
    ids = bits(aov1[..., 3])
    want = bits(motion[..., 3])
    py, px = np.mgrid[0:h, 0:w].astype(np.float64)
    with np.errstate(all="ignore"):
        zp = m[..., 2]
        live = np.isfinite(zp)
        qx, qy = px + 0.5 + m[..., 0] - 0.5, py + 0.5 + m[..., 1] - 0.5
        finite_q = np.isfinite(qx) & np.isfinite(qy)
        qx0, qy0 = np.where(finite_q, qx, -10.0), np.where(finite_q, qy, -10.0)
        x0, y0 = np.floor(qx0), np.floor(qy0)
        ax, ay = qx0 - x0, qy0 - y0
        gx, gy = _slope(z, 1), _slope(z, 0)
        fin_c = np.isfinite(c).all(-1)
        sw, acc = np.zeros((h, w)), np.zeros((h, w, 3))
        accepted = np.zeros((h, w, 4), bool)
        edge = (np.abs(qx0 - np.round(qx0)) <= 1e-4) | (np.abs(qy0 - np.round(qy0)) <= 1e-4)
        for t, (dy, dx) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
            tx, ty = x0 + dx, y0 + dy
            inside = finite_q & (tx >= 0) & (tx < w) & (ty >= 0) & (ty < h)
            ix, iy = np.clip(tx, 0, w - 1).astype(np.int64), np.clip(ty, 0, h - 1).astype(np.int64)
            wt = (ax if dx else 1.0 - ax) * (ay if dy else 1.0 - ay)
            zh = z[iy, ix] + (gx[iy, ix] * (qx0 - tx) + gy[iy, ix] * (qy0 - ty))
            others = live & inside & (ids[iy, ix] == want) & fin_c[iy, ix]
            ok = others & (np.abs(zh - zp) <= tol * zp)
            edge |= others & (np.abs(np.abs(zh - zp) / zp - tol) <= 1e-4 * tol)
            accepted[..., t] = ok
            sw += np.where(ok, wt, 0.0)
            acc += np.where(ok[..., None], wt[..., None] * np.where(fin_c[iy, ix][..., None], c[iy, ix], 0.0), 0.0)
        good = sw > 0
        out = np.zeros((h, w, 4))
        out[..., :3] = np.where(good[..., None], acc / np.where(good, sw, 1.0)[..., None], 0.0)
        out[..., 3] = np.where(good, sw, 0.0)
    return out, accepted, edge & live


def accepted_taps(reproject, motion, color, aov0, aov1, **params):
    """Which of its four taps an implementation accepted, per pixel (H x W x 4 bool, tap order), found from its outputs alone: the four taps
    of a pixel lie in the four parity classes of (x & 1, y & 1), so with a colour image that is 1 on one class and 0 elsewhere (and not
    finite wherever `color` is not) out.x * out.w is that tap's weight where it was accepted and 0 where it was not.  Only meaningful
    where every weight is > 0: away from a q on an integer."""
    h, w = motion.shape[:2]
    y, x = np.mgrid[0:h, 0:w]
    fin = np.isfinite(color[..., :3]).all(-1)
    share = np.zeros((2, 2, h, w))
    for cy in (0, 1):
        for cx in (0, 1):
            one_hot = np.where(fin & ((x & 1) == cx) & ((y & 1) == cy), 1.0, 0.0).astype(np.float32)
            image = np.repeat(np.where(fin, one_hot, np.float32(np.nan))[..., None], 4, -1).astype(np.float32)
            out = reproject(motion, image, aov0, aov1, **params)
            share[cy, cx] = out[..., 0].astype(np.float64) * out[..., 3]
    with np.errstate(all="ignore"):
        qx = (x + 0.5 + motion[..., 0].astype(np.float64)) - 0.5
        qy = (y + 0.5 + motion[..., 1].astype(np.float64)) - 0.5
        ok = np.isfinite(qx) & np.isfinite(qy)
        x0 = np.floor(np.where(ok, qx, 0.0)).astype(np.int64)
        y0 = np.floor(np.where(ok, qy, 0.0)).astype(np.int64)
    taps = np.zeros((h, w, 4), bool)
    for t, (dy, dx) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        taps[..., t] = share[(y0 + dy) & 1, (x0 + dx) & 1, y, x] > 0
    return taps


def reproject_inputs(width, height, seed, shift):
    """A synthetic previous frame (denoise_ref.synthetic_frame) and a motion plane for it: the given shift plus sub-pixel noise per pixel,
    z' = the previous depth at the nearest pixel to the target times (1 +- up to 3 %), so that taps both pass and fail the depth test at
    the default tolerance, the instance bits of that nearest pixel; then the planted cases: targets outside the frame, misses, z' = +inf,
    NaN and +-inf colours and motions, instance mismatches.  Returns motion, colour, aov0, aov1 (H x W x 4 float32)."""
    rng = np.random.default_rng(seed)
    color, aov0, aov1, _ = synthetic_frame(width, height, seed)
    y, x = np.mgrid[0:height, 0:width]
    mx = shift[0] + rng.uniform(-0.35, 0.35, (height, width))
    my = shift[1] + rng.uniform(-0.35, 0.35, (height, width))
    nx = np.clip(np.round(x + mx), 0, width - 1).astype(np.int64)
    ny = np.clip(np.round(y + my), 0, height - 1).astype(np.int64)
    zp = aov0[ny, nx, 3].astype(np.float64) * (1.0 + rng.uniform(-0.03, 0.03, (height, width)))
    motion = np.stack([mx, my, zp, np.zeros_like(zp)], -1).astype(np.float32)
    motion[..., 3] = aov1[ny, nx, 3]
    flat = rng.permutation(width * height)
    n = max(4, width * height // 200)
    pick = [np.unravel_index(flat[k * n:(k + 1) * n], (height, width)) for k in range(8)] if width * height >= 8 * n else []
    if pick:
        motion[pick[0] + (0,)] += np.float32(3.0 * width)                   # targets outside the frame
        motion[pick[1] + (1,)] -= np.float32(2.0 * height)
        motion[pick[2] + (2,)] = np.inf                                       # z' = +inf with live instance bits
        motion[pick[3]] = (0.0, 0.0, np.inf, MISS.view(np.float32))           # misses
        motion[pick[4] + (3,)] = np.uint32(7).view(np.float32)                # an instance no previous pixel has
        color[pick[5] + (0,)] = np.nan
        color[pick[6] + (1,)] = np.inf
        color[pick[7] + (2,)] = -np.inf
        motion[pick[5][0][:2], pick[5][1][:2], 0] = (np.nan, np.inf)          # motions that are not finite
        other = bits(aov1[..., 3]).copy()                                     # a block of the previous frame changes instance
        other[height // 2 + 2:height // 2 + 9, width // 3:width // 3 + 11] = 1 - np.minimum(other[height // 2 + 2:height // 2 + 9, width // 3:width // 3 + 11], 1)
        aov1[..., 3] = other.view(np.float32)
    return np.ascontiguousarray(motion), color, aov0, aov1
