"""The skinning rule on the host (glz_host_skin: the reference k_skin must match bit for bit) against the specification in
include/glaze_abi.h ("THE SKINNING RULE"), restated here in numpy: once in float32 with the operations in the specification's order (bit
for bit), once in float64 (within a bound derived from the operation count).  No device."""
import numpy as np
import pytest

import glaze_amd
from glaze_amd import abi

U = 2.0 ** -24          # the unit roundoff of float32


def restate(bind, joints, weights, bones, dtype):
    """the rule, operation by operation: numpy rounds every elementwise + and * of float32 arrays to float32"""
    v = np.asarray(bind, dtype)
    w = np.asarray(weights, dtype)
    B = np.asarray(bones, dtype).reshape(-1, 4, 4).transpose(0, 2, 1)          # [k][r][c] of the column-major matrices
    j = np.asarray(joints, np.int64)
    out = v.copy()
    with np.errstate(all="ignore"):
        for r in range(3):
            M = []
            for c in range(4):
                b = [B[j[:, i], r, c] for i in range(4)]
                M.append(((w[:, 0] * b[0] + w[:, 1] * b[1]) + w[:, 2] * b[2]) + w[:, 3] * b[3])
            out[:, r] = ((M[0] * v[:, 0] + M[1] * v[:, 1]) + M[2] * v[:, 2]) + M[3]
            out[:, 3 + r] = (M[0] * v[:, 3] + M[1] * v[:, 4]) + M[2] * v[:, 5]
    return out


def random_vertices(rng, n):
    v = rng.normal(size=(n, 8)).astype(np.float32)
    v[:, 3:6] /= np.linalg.norm(v[:, 3:6], axis=1, keepdims=True)
    return v


def random_bones(rng, k):
    """anything: rotation, scale and shear, translation, and a fourth row that must not matter"""
    m = rng.normal(size=(k, 4, 4)).astype(np.float32)
    m[:, 3, :] = rng.normal(size=(k, 4)) * 100.0
    return np.ascontiguousarray(m.transpose(0, 2, 1).reshape(k, 16), np.float32)


def rigid_bones(rng, k, reach=3.0):
    out = []
    for _ in range(k):
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        m = np.eye(4)
        m[:3, :3] = q * np.sign(np.linalg.det(q))
        m[:3, 3] = rng.uniform(-reach, reach, 3)
        out.append(m.T.reshape(16))
    return np.asarray(out, np.float32)


def random_influences(rng, n, k, convex=False):
    j = rng.integers(0, k, (n, 4))
    j[0] = (0, k - 1, 0, k - 1)                                                # bone 0 and the last one
    j[-1] = k - 1
    if convex:
        w = rng.random((n, 4))
        w[rng.random((n, 4)) < 0.3] = 0.0
        w[:, 0] += 1e-3
        w /= w.sum(1, keepdims=True)
    else:
        w = rng.normal(size=(n, 4))                                            # negative ones, sums that are not 1
        w[rng.random((n, 4)) < 0.3] = 0.0
    return j.astype(np.uint16), w.astype(np.float32)


def same_finite_bits(got, want):
    fg, fw = np.isfinite(got), np.isfinite(want)
    assert np.array_equal(fg, fw)                                              # the same set of non-finite outputs (payloads are not compared)
    assert np.array_equal(got.view(np.uint32)[fg], want.view(np.uint32)[fw])


@pytest.mark.parametrize("n,k", [(1, 1), (63, 2), (1000, 37), (257, 300)])
def test_host_skin_is_the_float32_restatement_bit_for_bit(n, k):
    rng = np.random.default_rng(n * 1000 + k)
    v, bones = random_vertices(rng, n), random_bones(rng, k)
    j, w = random_influences(rng, n, k)
    got = glaze_amd.host_skin(v, j, w, bones)
    assert np.isfinite(got).all()
    same_finite_bits(got, restate(v, j, w, bones, np.float32))
    assert np.array_equal(got[:, 6:].view(np.uint32), v[:, 6:].view(np.uint32))               # t' = t
    assert not np.array_equal(got[:, :6], v[:, :6])


def test_zero_weights_skip_nothing_and_non_finite_bones_reach_the_same_outputs():
    rng = np.random.default_rng(5)
    n, k = 400, 6
    v, bones = random_vertices(rng, n), random_bones(rng, k)
    j, w = random_influences(rng, n, k)
    bones[1, 0], bones[2, 13], bones[3, 6], bones[4, 15] = np.nan, np.inf, -np.inf, np.nan    # ([4, 15]: the fourth row, never read)
    got = glaze_amd.host_skin(v, j, w, bones)
    want = restate(v, j, w, bones, np.float32)
    same_finite_bits(got, want)
    assert (~np.isfinite(got)).any() and np.isfinite(got).any()
    zero_on_inf = ((j == 2) & (w == 0.0)).any(1)                                               # 0 x inf is NaN: the term is not skipped
    assert zero_on_inf.any() and np.isnan(got[zero_on_inf, 1]).all()
    only_four = (j == 4).all(1)
    if only_four.any():
        assert np.isfinite(got[only_four]).all()


def test_rigid_bones_with_convex_weights_stay_near_float64():
    rng = np.random.default_rng(11)
    n, k = 5000, 24
    v, bones = random_vertices(rng, n), rigid_bones(rng, k)
    j, w = random_influences(rng, n, k, convex=True)
    got = glaze_amd.host_skin(v, j, w, bones).astype(np.float64)
    exact = restate(v, j, w, bones, np.float64)
    # Every product w_i * B_i[r][c] * x_c reaches the result through at most 8 roundings (the product with the weight, three sums of the
    # blend, the product with the coordinate, three sums of the row), each of relative size U, so the error is at most
    # ((1 + U)^8 - 1) times the sum of the terms' magnitudes: 9 U L covers the second-order part.
    B = np.abs(bones.astype(np.float64).reshape(-1, 4, 4).transpose(0, 2, 1))[j.astype(np.int64)][:, :, :3, :]   # [n][i][r][c], r < 3
    wa = np.abs(w.astype(np.float64))[:, :, None]
    p = np.abs(v[:, :3].astype(np.float64))[:, None, None, :]
    nn = np.abs(v[:, 3:6].astype(np.float64))[:, None, None, :]
    L_pos = (wa * ((B[..., :3] * p).sum(-1) + B[..., 3])).sum(1)
    L_nrm = (wa * (B[..., :3] * nn).sum(-1)).sum(1)
    assert (np.abs(got[:, :3] - exact[:, :3]) <= 9 * U * L_pos).all()
    assert (np.abs(got[:, 3:6] - exact[:, 3:6]) <= 9 * U * L_nrm).all()
    assert np.abs(got[:, :3] - exact[:, :3]).max() > 0                                         # (float32 did round somewhere)
    one = (w == 1.0).any(1)                                                                     # under ONE rigid bone the normal keeps its length
    if one.any():
        assert np.linalg.norm(got[one, 3:6], axis=1) == pytest.approx(1.0, abs=1e-5)


def test_refused_arguments():
    lib = abi.lib()
    v = np.zeros((2, 8), np.float32)
    j = np.array([[0, 0, 0, 2]] * 2, np.uint16)
    w = np.ones((2, 4), np.float32)
    b = np.zeros((2, 16), np.float32)
    out = np.zeros_like(v)
    p = lambda a: a.ctypes.data
    assert lib.glz_host_skin(p(v), p(j), p(w), 2, p(b), 2, p(out)) == abi.E_ARG               # a joint past the bones
    assert lib.glz_host_skin(p(v), p(j), p(w), 2, p(b), 0, p(out)) == abi.E_ARG
    assert lib.glz_host_skin(p(v), p(j), p(w), 2, None, 3, p(out)) == abi.E_ARG
    assert lib.glz_host_skin(None, p(j), p(w), 2, p(b), 3, p(out)) == abi.E_ARG
    b3 = np.zeros((3, 16), np.float32)
    assert lib.glz_host_skin(p(v), p(j), p(w), 2, p(b3), 3, p(out)) == abi.OK
    assert lib.glz_host_skin(None, None, None, 0, p(b3), 3, None) == abi.OK
    with pytest.raises(ValueError):
        glaze_amd.host_skin(v, j[:1], w[:1], b3)


def test_the_header_states_the_rule():
    import os
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "glaze_abi.h")).read()
    for piece in ("THE SKINNING RULE", "M[r][c] = ((w0 * B[j0][r][c] + w1 * B[j1][r][c]) + w2 * B[j2][r][c]) + w3 * B[j3][r][c]",
                  "p'[r]   = ((M[r][0] * p.x + M[r][1] * p.y) + M[r][2] * p.z) + M[r][3]", "n'[r]   =  (M[r][0] * n.x + M[r][1] * n.y) + M[r][2] * n.z",
                  "exact only for rigid bones"):
        assert piece in text, piece
