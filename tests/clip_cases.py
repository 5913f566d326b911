"""What tests/test_clip_host.py and tests/test_gpu_clip.py share: THE CLIP RULE of include/glaze_abi.h restated in numpy float32, one
operation per numpy call in the specification's order -- written from that comment, not from the C++ -- and seeded skeletons and clips."""
import numpy as np

F = np.float32


def key_choice(times, t):
    """step 1, in float32: (k0, k1, u)"""
    times, t = np.asarray(times, F), F(t)
    last = len(times) - 1
    if t <= times[0]:
        return 0, 0, F(0)
    if t >= times[last]:
        return last, last, F(0)
    k0 = max(k for k in range(len(times)) if times[k] <= t)
    return k0, k0 + 1, (t - times[k0]) / (times[k0 + 1] - times[k0])


def lerp(a, b, u):
    return a + u * (b - a)


def product(A, B):
    """step 5 on (3, 4) float32 arrays"""
    C = np.empty((3, 4), F)
    for c in range(3):
        C[:, c] = (A[:, 0] * B[0, c] + A[:, 1] * B[1, c]) + A[:, 2] * B[2, c]
    C[:, 3] = ((A[:, 0] * B[0, 3] + A[:, 1] * B[1, 3]) + A[:, 2] * B[2, 3]) + A[:, 3]
    return C


def upper(m16):
    """the upper 3 x 4, [r][c], of a column-major matrix"""
    return np.asarray(m16, F).reshape(4, 4).T[:3].copy()


def restate(parents, inverse_bind, times, translations, rotations, time, scales=None, morph_weights=None, root=None):
    """steps 1 - 6: ((n_bones, 16) float32 bones with the fourth row (0, 0, 0, 1), the lerped weights or None)"""
    tr, ro = np.asarray(translations, F), np.asarray(rotations, F)
    n = tr.shape[1]
    k0, k1, u = key_choice(times, time)
    one, two = F(1), F(2)
    with np.errstate(all="ignore"):
        t = lerp(tr[k0], tr[k1], u)
        s = np.ones((n, 3), F) if scales is None else lerp(np.asarray(scales, F)[k0], np.asarray(scales, F)[k1], u)
        a, b = ro[k0], ro[k1].copy()
        dot = ((a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]) + a[:, 3] * b[:, 3]
        b[dot < 0] = -b[dot < 0]
        Q = lerp(a, b, u)
        nn = ((Q[:, 0] * Q[:, 0] + Q[:, 1] * Q[:, 1]) + Q[:, 2] * Q[:, 2]) + Q[:, 3] * Q[:, 3]
        inv = one / np.sqrt(nn)
        q = Q * inv[:, None]
        x, y, z, w = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
        xx, yy, zz, xy, xz, yz, wx, wy, wz = x * x, y * y, z * z, x * y, x * z, y * z, w * x, w * y, w * z
        L = np.empty((n, 3, 4), F)
        L[:, 0, 0], L[:, 0, 1], L[:, 0, 2] = (one - two * (yy + zz)) * s[:, 0], (two * (xy - wz)) * s[:, 1], (two * (xz + wy)) * s[:, 2]
        L[:, 1, 0], L[:, 1, 1], L[:, 1, 2] = (two * (xy + wz)) * s[:, 0], (one - two * (xx + zz)) * s[:, 1], (two * (yz - wx)) * s[:, 2]
        L[:, 2, 0], L[:, 2, 1], L[:, 2, 2] = (two * (xz - wy)) * s[:, 0], (two * (yz + wx)) * s[:, 1], (one - two * (xx + yy)) * s[:, 2]
        L[:, :, 3] = t
        R = upper(np.eye(4, dtype=F).T.reshape(16) if root is None else root)
        W, out = [], np.zeros((n, 16), F)
        for bone in range(n):
            W.append(product(R if parents[bone] < 0 else W[parents[bone]], L[bone]))
            B = product(W[bone], upper(np.asarray(inverse_bind, F).reshape(-1, 16)[bone]))
            out[bone] = np.vstack([B, np.array([[0, 0, 0, 1]], F)]).T.reshape(16)
        weights = None if morph_weights is None else lerp(np.asarray(morph_weights, F)[k0], np.asarray(morph_weights, F)[k1], u)
    return out, weights


def pack_rows(bones):
    """pack_bone of (n, 16) column-major matrices: (n, 12), the three rows of each"""
    b = np.asarray(bones, F).reshape(-1, 4, 4)   # [c][r]
    return np.ascontiguousarray(b.transpose(0, 2, 1)[:, :3, :]).reshape(-1, 12)


# ---- seeded skeletons and clips ---------------------------------------------------------------------------------------------------
def chain(n):
    return np.arange(-1, n - 1, dtype=np.int32)


def star(n):
    """bone 0 the root, every other bone its child: two levels"""
    p = np.zeros(n, np.int32)
    p[0] = -1
    return p


def random_tree(rng, n, roots=1):
    p = np.full(n, -1, np.int32)
    for b in range(roots, n):
        p[b] = rng.integers(0, b)
    return p


def random_rigid(rng, n, reach=1.0):
    """n column-major rigid matrices: a random rotation and a translation within `reach`"""
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    x, y, z, w = q.T
    m = np.zeros((n, 4, 4))
    m[:, 0, 0], m[:, 0, 1], m[:, 0, 2] = 1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)
    m[:, 1, 0], m[:, 1, 1], m[:, 1, 2] = 2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)
    m[:, 2, 0], m[:, 2, 1], m[:, 2, 2] = 2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)
    m[:, :3, 3] = rng.uniform(-reach, reach, size=(n, 3))
    m[:, 3, 3] = 1
    return np.ascontiguousarray(m.transpose(0, 2, 1)).reshape(n, 16).astype(F)


def random_clip(rng, n_bones, n_keys, scaled=True, n_targets=0, reach=0.25, turn=0.3):
    """A clip of small motions (a deep chain stays bounded): times, translations, rotations (not normalised: the rule takes them as given),
    scales or None, morph weights or None"""
    times = np.cumsum(rng.uniform(0.25, 1.0, n_keys)).astype(F)
    tr = rng.uniform(-reach, reach, (n_keys, n_bones, 3)).astype(F)
    ro = np.concatenate([rng.normal(0, turn, (n_keys, n_bones, 3)), rng.uniform(0.8, 1.2, (n_keys, n_bones, 1)) * rng.choice([-1.0, 1.0], (n_keys, n_bones, 1))], -1).astype(F)
    sc = rng.uniform(0.9, 1.1, (n_keys, n_bones, 3)).astype(F) if scaled else None
    mw = rng.uniform(-0.5, 1.0, (n_keys, n_targets)).astype(F) if n_targets else None
    return times, tr, ro, sc, mw


def times_around(times):
    """before the first key, on every key, between every pair, after the last"""
    times = np.asarray(times, F)
    between = [F(times[k] + F(0.37) * (times[k + 1] - times[k])) for k in range(len(times) - 1)]
    return [F(times[0] - 1)] + [F(t) for t in times] + between + [F(times[-1] + 1)]
