"""The dual-quaternion rule on the host (glz_host_bone_dual_quats, glz_host_skin_dq: the reference k_skin_dq must match bit for bit)
against the specification in include/glaze_abi.h ("THE DUAL-QUATERNION RULE"), restated here in numpy: the bone conversion in float64, one
bone at a time, and the per-vertex rule in float32 with one operation per numpy call, both in the specification's order (bit for bit); and
against float64 and closed forms (a twist keeps its radius, a hinge keeps its axis).  No device."""
import os

import numpy as np
import pytest

import glaze_amd
from glaze_amd import abi

from test_skin_host import random_bones, random_influences, random_vertices, same_finite_bits

F = np.float64


# ---- the rule, restated ---------------------------------------------------------------------------------------------------------
def restate_bone(m16):
    """BONE CONVERSION of the header on one column-major matrix: (8 float32, the Shepperd branch taken)"""
    m = [[F(m16[4 * c + r]) for c in range(4)] for r in range(4)]
    one, two, four, half = F(1), F(2), F(4), F(0.5)
    with np.errstate(all="ignore"):
        tr = (m[0][0] + m[1][1]) + m[2][2]
        if tr > 0:
            branch = 0
            s = two * np.sqrt(tr + one)
            w, x, y, z = s / four, (m[2][1] - m[1][2]) / s, (m[0][2] - m[2][0]) / s, (m[1][0] - m[0][1]) / s
        elif m[0][0] > m[1][1] and m[0][0] > m[2][2]:
            branch = 1
            s = two * np.sqrt(((one + m[0][0]) - m[1][1]) - m[2][2])
            w, x, y, z = (m[2][1] - m[1][2]) / s, s / four, (m[0][1] + m[1][0]) / s, (m[0][2] + m[2][0]) / s
        elif m[1][1] > m[2][2]:
            branch = 2
            s = two * np.sqrt(((one + m[1][1]) - m[0][0]) - m[2][2])
            w, x, y, z = (m[0][2] - m[2][0]) / s, (m[0][1] + m[1][0]) / s, s / four, (m[1][2] + m[2][1]) / s
        else:
            branch = 3
            s = two * np.sqrt(((one + m[2][2]) - m[0][0]) - m[1][1])
            w, x, y, z = (m[1][0] - m[0][1]) / s, (m[0][2] + m[2][0]) / s, (m[1][2] + m[2][1]) / s, s / four
        ln = np.sqrt(((x * x + y * y) + z * z) + w * w)
        x, y, z, w = x / ln, y / ln, z / ln, w / ln
        tx, ty, tz = m[0][3], m[1][3], m[2][3]
        dx = half * ((tx * w + ty * z) - tz * y)
        dy = half * ((ty * w + tz * x) - tx * z)
        dz = half * ((tz * w + tx * y) - ty * x)
        dw = -(half * ((tx * x + ty * y) + tz * z))
        return np.array([x, y, z, w, dx, dy, dz, dw], np.float64).astype(np.float32), branch


def restate_bones(bones):
    rows = [restate_bone(b) for b in np.asarray(bones, np.float32).reshape(-1, 16)]
    return np.stack([r[0] for r in rows]), [r[1] for r in rows]


def restate_vertices(bind, joints, weights, dq, signs=True):
    """PER VERTEX of the header on converted bones dq (k, 8) float32: numpy rounds every elementwise + - * / sqrt of float32 arrays to
    float32.  signs=False leaves step 1 out (what the sign step is compared with)."""
    v = np.asarray(bind, np.float32).reshape(-1, 8)
    w = np.asarray(weights, np.float32)
    j = np.asarray(joints, np.int64)
    dq = np.asarray(dq, np.float32)
    one, two = np.float32(1), np.float32(2)
    X, Y, Z, W = 0, 1, 2, 3
    with np.errstate(all="ignore"):
        q = [[dq[j[:, k], e] for e in range(4)] for k in range(4)]
        d = [[dq[j[:, k], 4 + e] for e in range(4)] for k in range(4)]
        c = [w[:, 0]]
        for k in (1, 2, 3):
            dot = ((q[0][X] * q[k][X] + q[0][Y] * q[k][Y]) + q[0][Z] * q[k][Z]) + q[0][W] * q[k][W]
            c.append(np.where(dot < 0, -w[:, k], w[:, k]) if signs else w[:, k])
        R = [((c[0] * q[0][e] + c[1] * q[1][e]) + c[2] * q[2][e]) + c[3] * q[3][e] for e in range(4)]
        D = [((c[0] * d[0][e] + c[1] * d[1][e]) + c[2] * d[2][e]) + c[3] * d[3][e] for e in range(4)]
        nn = ((R[X] * R[X] + R[Y] * R[Y]) + R[Z] * R[Z]) + R[W] * R[W]
        inv = one / np.sqrt(nn)
        r = [R[e] * inv for e in range(4)]
        dd = [D[e] * inv for e in range(4)]
        nxt, prv = (Y, Z, X), (Z, X, Y)                                                          # x -> y -> z -> x
        T = [two * (((r[W] * dd[e] - dd[W] * r[e]) + r[nxt[e]] * dd[prv[e]]) - r[prv[e]] * dd[nxt[e]]) for e in range(3)]

        def rot(u):
            a = [(r[nxt[e]] * u[prv[e]] - r[prv[e]] * u[nxt[e]]) + r[W] * u[e] for e in range(3)]
            b = [r[nxt[e]] * a[prv[e]] - r[prv[e]] * a[nxt[e]] for e in range(3)]
            return [u[e] + two * b[e] for e in range(3)]

        p, n = rot([v[:, 0], v[:, 1], v[:, 2]]), rot([v[:, 3], v[:, 4], v[:, 5]])
        out = v.copy()
        for e in range(3):
            out[:, e] = p[e] + T[e]
            out[:, 3 + e] = n[e]
    assert out.dtype == np.float32 and nn.dtype == np.float32
    return out


def restate(bind, joints, weights, bones, signs=True):
    return restate_vertices(bind, joints, weights, restate_bones(bones)[0], signs)


def col_major(m):
    return np.ascontiguousarray(np.asarray(m, np.float64).T.reshape(16), np.float32)


def about_x(angle, y=0.0, z=0.0):
    """a rotation about the line through (., y, z) parallel to x, as float64 4 x 4"""
    c, s = np.cos(angle), np.sin(angle)
    m = np.eye(4)
    m[1:3, 1:3] = [[c, -s], [s, c]]
    m[1:3, 3] = np.array([y, z]) - m[1:3, 1:3] @ np.array([y, z])
    return m


def turned_bones(rng, k, reach=3.0):
    """rigid bones whose rotations are uniform over all rotations (a normalised gaussian quaternion), so that every Shepperd branch is
    reached; test_skin_host.rigid_bones' QR factors rarely have their largest diagonal element in the middle"""
    out = []
    for _ in range(k):
        x, y, z, w = (lambda q: q / np.linalg.norm(q))(rng.normal(size=4))
        m = np.eye(4)
        m[:3, :3] = [[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]
        m[:3, 3] = rng.uniform(-reach, reach, 3)
        out.append(m.T.reshape(16))
    return np.asarray(out, np.float32)


def scaled_bones(rng, k):
    """test_gpu_skin.py's random_bones: near the identity, with scale and shear, and a fourth row that is never read"""
    m = np.tile(np.eye(4), (k, 1, 1))
    m[:, :3, :3] += rng.normal(size=(k, 3, 3)) * 0.15
    m[:, :3, 3] = rng.uniform(-0.1, 0.1, (k, 3))
    m[:, 3, :] = rng.normal(size=(k, 4))
    return np.ascontiguousarray(m.transpose(0, 2, 1).reshape(k, 16), np.float32)


# ---- bit equality ---------------------------------------------------------------------------------------------------------------
def test_rigid_bones_reach_every_shepperd_branch_and_convert_bit_for_bit():
    rng = np.random.default_rng(1)
    bones = turned_bones(rng, 400)
    want, branches = restate_bones(bones)
    assert set(branches) == {0, 1, 2, 3}
    got = glaze_amd.host_bone_dual_quats(bones)
    assert np.isfinite(got).all()
    same_finite_bits(got, want)
    assert np.linalg.norm(got[:, :4].astype(np.float64), axis=1) == pytest.approx(1.0, abs=2e-7)


@pytest.mark.parametrize("kind", ["rigid", "anything", "scaled"])
@pytest.mark.parametrize("n,k", [(1, 1), (63, 2), (1000, 37), (257, 300)])
def test_host_skin_dq_is_the_restatement_bit_for_bit(n, k, kind):
    rng = np.random.default_rng(n * 1000 + k)
    v = random_vertices(rng, n)
    bones = {"rigid": turned_bones, "anything": random_bones, "scaled": scaled_bones}[kind](rng, k)
    j, w = random_influences(rng, n, k)                                                          # negative weights, zeros, sums that are not 1
    dq, branches = restate_bones(bones)
    if kind == "rigid" and k >= 37:
        assert set(branches) == {0, 1, 2, 3}
    same_finite_bits(glaze_amd.host_bone_dual_quats(bones), dq)
    got = glaze_amd.host_skin(v, j, w, bones, blend="dual_quaternion")
    same_finite_bits(got, restate_vertices(v, j, w, dq))
    assert np.array_equal(got[:, 6:].view(np.uint32), v[:, 6:].view(np.uint32))                  # t' = t
    assert not np.array_equal(got[:, :6], v[:, :6])
    # out may be bind itself
    alias = v.copy()
    assert abi.lib().glz_host_skin_dq(alias.ctypes.data, j.ctypes.data, w.ctypes.data, n, bones.ctypes.data, k, alias.ctypes.data) == abi.OK
    assert np.array_equal(alias.view(np.uint32), got.view(np.uint32))


def test_the_sign_step_negates_the_weight_of_a_bone_on_the_other_hemisphere():
    """+100 and -100 degrees about one axis: the quaternions' dot is cos(100 degrees) = -0.17, so the second weight is negated"""
    bones = np.stack([col_major(about_x(np.radians(100.0))), col_major(about_x(np.radians(-100.0)))])
    dq = glaze_amd.host_bone_dual_quats(bones)
    assert float(dq[0, :4].astype(np.float64) @ dq[1, :4].astype(np.float64)) == pytest.approx(np.cos(np.radians(100.0)), abs=1e-6)
    rng = np.random.default_rng(2)
    n = 64
    v = random_vertices(rng, n)
    j = np.tile(np.array([0, 1, 1, 0], np.uint16), (n, 1))
    w = np.zeros((n, 4), np.float32)
    w[:, 0] = rng.uniform(0.2, 0.8, n)
    w[:, 1] = 1.0 - w[:, 0]
    got = glaze_amd.host_skin(v, j, w, bones, blend="dual_quaternion")
    same_finite_bits(got, restate(v, j, w, bones))
    assert not np.array_equal(got, restate(v, j, w, bones, signs=False))
    # with the pivot swapped the result is the same motion: q and -q are one rotation
    swapped = glaze_amd.host_skin(v, j[:, ::-1].copy(), w[:, [3, 2, 1, 0]].copy(), bones, blend="dual_quaternion")
    assert np.abs(swapped - got).max() < 1e-5


def half_turn(axis, minus_zero=()):
    """diag(+-1): the half turn about `axis`, whose conversion is exactly the unit quaternion of that axis; the off-diagonal elements
    named in minus_zero (pairs (r, c)) are -0.0 instead of +0.0, which the conversion carries into the quaternion's zeros"""
    m = np.zeros((4, 4), np.float32)
    for a in range(3):
        m[a, a] = 1.0 if a == axis else -1.0
    m[3, 3] = 1.0
    for r, c in minus_zero:
        m[r, c] = -0.0
    return np.ascontiguousarray(m.T.reshape(16))


def test_a_dot_of_exactly_zero_of_either_sign_keeps_the_weight():
    plus = np.stack([half_turn(0), half_turn(1)])                                                # (1, 0, 0, 0) and (0, 1, 0, 0)
    issue = np.stack([half_turn(0), half_turn(1, [(0, 1), (1, 0)])])                             # (1, 0, 0, 0) and (-0, 1, 0, 0)
    # every product of the dot -0: q0 = (1, -0, -0, -0) against (-0, 1, 0, 0)
    minus = np.stack([half_turn(0, [(0, 1), (1, 0), (0, 2), (2, 0), (2, 1)]), half_turn(1, [(0, 1), (1, 0)])])
    f32 = np.float32
    bits = lambda a: np.asarray(a, np.float32).view(np.uint32).tolist()
    want_q = {id(plus): ([1, 0, 0, 0], [0, 1, 0, 0]), id(issue): ([1, 0, 0, 0], [-0.0, 1, 0, 0]), id(minus): ([1, -0.0, -0.0, -0.0], [-0.0, 1, 0, 0])}
    rng = np.random.default_rng(3)
    n = 32
    v = random_vertices(rng, n)
    j = np.tile(np.array([0, 1, 0, 0], np.uint16), (n, 1))
    w = np.zeros((n, 4), np.float32)
    w[:, 0], w[:, 1] = 0.75, 0.25
    results = []
    for bones in (plus, issue, minus):
        dq = glaze_amd.host_bone_dual_quats(bones)
        assert bits(dq[0, :4]) == bits(want_q[id(bones)][0]) and bits(dq[1, :4]) == bits(want_q[id(bones)][1])
        q0, q1 = dq[0, :4], dq[1, :4]
        dot = ((q0[0] * q1[0] + q0[1] * q1[1]) + q0[2] * q1[2]) + q0[3] * q1[3]
        assert dot == 0 and dot.dtype == np.float32
        assert bool(np.signbit(dot)) == (bones is minus)                                         # (-0 + +0 is +0: only all four products at -0 sum to -0)
        got = glaze_amd.host_skin(v, j, w, bones, blend="dual_quaternion")
        same_finite_bits(got, restate(v, j, w, bones))
        same_finite_bits(got, restate(v, j, w, bones, signs=False))                              # the weight kept its sign
        results.append(got)
    negated = w.copy()
    negated[:, 1] = -0.25
    assert not np.array_equal(results[0], glaze_amd.host_skin(v, j, negated, plus, blend="dual_quaternion"))   # (and its sign does matter)
    assert np.abs(results[0] - results[2]).max() == 0


def test_non_finite_bones_and_a_zero_blend_give_the_same_non_finite_vertices():
    rng = np.random.default_rng(5)
    n, k = 400, 6
    v, bones = random_vertices(rng, n), turned_bones(rng, k)
    j, w = random_influences(rng, n, k)
    j[::5] = 0                                                                                   # a fifth of the vertices under the finite bone 0 alone
    bones[1, 0], bones[2, 13], bones[3, 6], bones[4, 15] = np.nan, np.inf, -np.inf, np.nan      # ([4, 15]: the fourth row, never read)
    dq = glaze_amd.host_bone_dual_quats(bones)
    same_finite_bits(dq, restate_bones(bones)[0])
    assert np.isfinite(dq[[0, 4, 5]]).all() and not np.isfinite(dq[[1, 2, 3]]).all()
    got = glaze_amd.host_skin(v, j, w, bones, blend="dual_quaternion")
    same_finite_bits(got, restate(v, j, w, bones))
    assert (~np.isfinite(got)).any() and np.isfinite(got[::5][np.abs(w[::5]).sum(1) > 0]).all()
    # weights (1, -1, 0, 0) on one bone: nn = 0, inv = inf, the vertex is not finite -- on both sides
    j0 = np.zeros((8, 4), np.uint16)
    w0 = np.tile(np.array([1, -1, 0, 0], np.float32), (8, 1))
    zero = glaze_amd.host_skin(v[:8], j0, w0, bones, blend="dual_quaternion")
    same_finite_bits(zero, restate(v[:8], j0, w0, bones))
    assert not np.isfinite(zero[:, :6]).any() and np.array_equal(zero[:, 6:], v[:8, 6:])


# ---- what the rule is worth -----------------------------------------------------------------------------------------------------
def test_one_rigid_bone_stays_near_float64():
    """One rigid bone at weight 1, its matrix in float64: 2 000 random rotations, |t| <= 1 and |p| <= 1 per axis.  The bound, 8e-6, was set
    by the numpy restatement of the rule alone, not by the library: its worst absolute error on this family measured 1.8e-6, and the
    bound is about four times that, for other draws."""
    rng = np.random.default_rng(17)
    n = 2000
    m64 = np.tile(np.eye(4), (n, 1, 1))
    for i in range(n):
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        m64[i, :3, :3] = q * np.sign(np.linalg.det(q))
    m64[:, :3, 3] = rng.uniform(-1, 1, (n, 3))
    bones = np.ascontiguousarray(m64.transpose(0, 2, 1).reshape(n, 16), np.float32)
    v = random_vertices(rng, n)
    v[:, :3] = rng.uniform(-1, 1, (n, 3))
    j = np.repeat(np.arange(n, dtype=np.uint16)[:, None], 4, 1)
    w = np.tile(np.array([1, 0, 0, 0], np.float32), (n, 1))
    got = glaze_amd.host_skin(v, j, w, bones, blend="dual_quaternion").astype(np.float64)
    p = np.einsum("nrc,nc->nr", m64[:, :3, :3], v[:, :3].astype(np.float64)) + m64[:, :3, 3]    # the float64 matrices, before rounding
    nrm = np.einsum("nrc,nc->nr", m64[:, :3, :3], v[:, 3:6].astype(np.float64))
    err_p, err_n = np.abs(got[:, :3] - p).max(), np.abs(got[:, 3:6] - nrm).max()
    print("worst absolute error: position %.3g, normal %.3g" % (err_p, err_n))
    assert err_p <= 8e-6 and err_n <= 8e-6


@pytest.mark.parametrize("angle", [np.pi / 2, 0.9 * np.pi, 0.999 * np.pi])
def test_a_twist_keeps_its_radius_where_linear_blending_collapses(angle):
    """two bones `angle` apart about x (one stays, one turns), weights 1/2 : 1/2, points at radius 1: the dual-quaternion blend turns
    them by half the angle on their circle (the restatement gave radii 1.0, 0.9999999 and 1.0, and |n'| >= 0.99999994); the linear blend
    pulls them in to cos(angle / 2): 0.707, 0.156, 0.0016"""
    bones = np.stack([col_major(np.eye(4)), col_major(about_x(angle))])
    v = np.array([[0.3, 1.0, 0.0, 0.0, 1.0, 0.0, 0.5, 0.5], [-0.2, 0.0, 1.0, 0.0, 0.0, 1.0, 0.1, 0.9]], np.float32)
    j = np.tile(np.array([0, 1, 0, 0], np.uint16), (2, 1))
    w = np.tile(np.array([0.5, 0.5, 0, 0], np.float32), (2, 1))
    dq = glaze_amd.host_skin(v, j, w, bones, blend="dual_quaternion").astype(np.float64)
    same_finite_bits(dq.astype(np.float32), restate(v, j, w, bones))
    radius, normal = np.hypot(dq[:, 1], dq[:, 2]), np.linalg.norm(dq[:, 3:6], axis=1)
    print("twist %.4f: radius %s, |n'| %s" % (angle, radius, normal))
    assert np.abs(radius - 1.0).max() <= 1e-6 and np.abs(normal - 1.0).max() <= 1e-6
    assert np.array_equal(dq[:, 0].astype(np.float32), v[:, 0])                                  # along the axis nothing moves
    # the point is turned by half the angle
    assert dq[0, 1] == pytest.approx(np.cos(angle / 2), abs=1e-6) and dq[0, 2] == pytest.approx(np.sin(angle / 2), abs=1e-6)
    lin = glaze_amd.host_skin(v, j, w, bones).astype(np.float64)                                 # the defect the mode exists for
    assert np.hypot(lin[:, 1], lin[:, 2]) == pytest.approx(np.cos(angle / 2), abs=1e-6)
    assert np.linalg.norm(lin[:, 3:6], axis=1) == pytest.approx(np.cos(angle / 2), abs=1e-6)


def test_a_hinge_keeps_the_points_of_its_axis():
    """the hinge of test_gpu_skin.py (the axis through y = -0.4, z = 0.55, parallel to x): a point on the axis stays within 2e-7 under
    any weights between the fixed bone and the turned one (the restatement measured 7e-8)"""
    rng = np.random.default_rng(23)
    n = 200
    bones = np.stack([col_major(np.eye(4)), col_major(about_x(0.5, -0.4, 0.55))])
    v = random_vertices(rng, n)
    v[:, 0] = rng.uniform(-0.5, 0.5, n)
    v[:, 1], v[:, 2] = -0.4, 0.55
    j = np.tile(np.array([0, 1, 1, 0], np.uint16), (n, 1))
    s = rng.random(n).astype(np.float32)
    w = np.stack([1 - s, s, np.zeros_like(s), np.zeros_like(s)], -1).astype(np.float32)
    got = glaze_amd.host_skin(v, j, w, bones, blend="dual_quaternion")
    same_finite_bits(got, restate(v, j, w, bones))
    moved = np.abs(got[:, :3].astype(np.float64) - v[:, :3].astype(np.float64)).max()
    print("hinge: a point of the axis moves by at most %.3g" % moved)
    assert moved <= 2e-7
    assert np.linalg.norm(got[:, 3:6].astype(np.float64), axis=1) == pytest.approx(1.0, abs=1e-6)


# ---- refused arguments ----------------------------------------------------------------------------------------------------------
def test_refused_arguments():
    lib = abi.lib()
    v = np.zeros((2, 8), np.float32)
    j = np.array([[0, 0, 0, 2]] * 2, np.uint16)
    w = np.ones((2, 4), np.float32)
    b = np.zeros((2, 16), np.float32)
    out = np.zeros_like(v)
    p = lambda a: a.ctypes.data
    assert lib.glz_host_skin_dq(p(v), p(j), p(w), 2, p(b), 2, p(out)) == abi.E_ARG              # a joint past the bones
    assert lib.glz_host_skin_dq(p(v), p(j), p(w), 2, p(b), 0, p(out)) == abi.E_ARG
    assert lib.glz_host_skin_dq(p(v), p(j), p(w), 2, None, 3, p(out)) == abi.E_ARG
    assert lib.glz_host_skin_dq(None, p(j), p(w), 2, p(b), 3, p(out)) == abi.E_ARG
    assert lib.glz_host_skin_dq(p(v), None, p(w), 2, p(b), 3, p(out)) == abi.E_ARG
    assert lib.glz_host_skin_dq(p(v), p(j), None, 2, p(b), 3, p(out)) == abi.E_ARG
    assert lib.glz_host_skin_dq(p(v), p(j), p(w), 2, p(b), 3, None) == abi.E_ARG
    b3 = np.zeros((3, 16), np.float32)
    assert lib.glz_host_skin_dq(p(v), p(j), p(w), 2, p(b3), 3, p(out)) == abi.OK
    assert lib.glz_host_skin_dq(None, None, None, 0, p(b3), 3, None) == abi.OK
    out8 = np.zeros((3, 8), np.float32)
    assert lib.glz_host_bone_dual_quats(None, 3, p(out8)) == abi.E_ARG and lib.glz_host_bone_dual_quats(p(b3), 3, None) == abi.E_ARG
    assert lib.glz_host_bone_dual_quats(None, 0, None) == abi.OK
    assert lib.glz_renderer_set_skin_blend(None, 0, abi.SKIN_DUAL_QUATERNION) == abi.E_ARG      # no renderer (the rest: test_gpu_skin_dq.py)
    assert lib.glz_renderer_skin_blend(None, 0) == abi.E_ARG
    with pytest.raises(ValueError):
        glaze_amd.host_skin(v, j[:1], w[:1], b3, blend="dual_quaternion")
    with pytest.raises(ValueError):
        glaze_amd.host_skin(v, j, w, b3, blend="quaternion")


def test_the_header_states_the_rule():
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "glaze_abi.h")).read()
    for piece in ("THE DUAL-QUATERNION RULE", "s = 2 * sqrt(tr + 1)", "dw = -(0.5 * ((tx * x + ty * y) + tz * z))",
                  "dot_k = ((q0.x * qk.x + q0.y * qk.y) + q0.z * qk.z) + q0.w * qk.w", "c_k = -w_k if dot_k < 0 else w_k",
                  "nn = ((R.x * R.x + R.y * R.y) + R.z * R.z) + R.w * R.w", "T.x = 2 * (((r.w * d.x - d.w * r.x) + r.y * d.z) - r.z * d.y)",
                  "a.x = (r.y * v.z - r.z * v.y) + r.w * v.x", "b.x = r.y * a.z - r.z * a.y", "nn == 0 is NOT special-cased", "GLZ_SKIN_DUAL_QUATERNION"):
        assert piece in text, piece
