"""The morph rule on the host (glz_host_morph: the reference k_morph and k_morph_skin must match bit for bit) against the specification in
include/glaze_abi.h ("THE MORPH RULE"), restated here in numpy: once in float32 with the operations in the specification's order (bit for
bit), once in float64 (within a bound derived from the operation count).  glz_host_morph runs through the layout packer the device path
uses, so these cases hold the packer to the rule as well.  No device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import glaze_amd
from glaze_amd import abi

U = 2.0 ** -24          # the unit roundoff of float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def restate(base, targets, weights, dtype):
    """the rule, operation by operation: numpy rounds every elementwise + and * of float32 arrays to float32.  Targets are taken in
    ascending order and each touches a vertex at most once, so every vertex sees its terms in the rule's order."""
    out = np.asarray(base, dtype).copy()
    w = np.asarray(weights, dtype)
    with np.errstate(all="ignore"):
        for t, (idx, dp, dn) in enumerate(targets):
            rows = np.arange(len(out)) if idx is None else np.asarray(idx, np.int64)
            out[rows, 0:3] = out[rows, 0:3] + w[t] * np.asarray(dp, dtype).reshape(-1, 3)
            out[rows, 3:6] = out[rows, 3:6] + w[t] * np.asarray(dn, dtype).reshape(-1, 3)
    return out


def row_lengths(n, targets):
    k = np.zeros(n, np.int64)
    for idx, _, _ in targets:
        k[np.arange(n) if idx is None else np.asarray(idx, np.int64)] += 1
    return k


def random_vertices(rng, n):
    v = rng.normal(size=(n, 8)).astype(np.float32)
    v[:, 3:6] /= np.linalg.norm(v[:, 3:6], axis=1, keepdims=True)
    return v


def random_target(rng, n, m, scale=0.1):
    """a sparse target over n vertices with m entries (m = None: dense, no index list)"""
    idx = None if m is None else np.sort(rng.choice(n, m, replace=False)).astype(np.uint32)
    k = n if m is None else m
    return idx, (rng.normal(size=(k, 3)) * scale).astype(np.float32), (rng.normal(size=(k, 3)) * scale).astype(np.float32)


def random_targets(rng, n, n_targets, per_target, dense=(), empty=()):
    return [random_target(rng, n, None if t in dense else 0 if t in empty else per_target) for t in range(n_targets)]


def random_weights(rng, n_targets):
    w = rng.normal(size=n_targets).astype(np.float32)                          # negative ones, sums that are not 1
    w[rng.random(n_targets) < 0.2] = 0.0
    return w


def same_finite_bits(got, want):
    fg, fw = np.isfinite(got), np.isfinite(want)
    assert np.array_equal(fg, fw)                                              # the same set of non-finite outputs (payloads are not compared)
    assert np.array_equal(got.view(np.uint32)[fg], want.view(np.uint32)[fw])


def cases():
    """(n, T) of the issue: (1, 1) dense; (63, 2) sparse; (1000, 37) a tenth of the vertices per target; (257, 300) a dense target, sparse
    ones and an empty one"""
    rng = np.random.default_rng(4)
    return [(1, random_targets(rng, 1, 1, 1, dense=(0,))), (63, random_targets(rng, 63, 2, 9)), (1000, random_targets(rng, 1000, 37, 100)),
            (257, random_targets(rng, 257, 300, 26, dense=(5,), empty=(0, 299)))]


@pytest.mark.parametrize("n,targets", cases(), ids=lambda x: str(x) if isinstance(x, int) else "T%d" % len(x))
def test_host_morph_is_the_float32_restatement_bit_for_bit(n, targets):
    rng = np.random.default_rng(1000 * n + len(targets))
    v, w = random_vertices(rng, n), random_weights(rng, len(targets))
    if len(targets) <= 2:
        w[:] = (0.75, -1.5)[:len(targets)]
    got = glaze_amd.host_morph(v, targets, w)
    assert np.isfinite(got).all()
    same_finite_bits(got, restate(v, targets, w, np.float32))
    assert np.array_equal(got[:, 6:].view(np.uint32), v[:, 6:].view(np.uint32))               # t' = t
    untouched = row_lengths(n, targets) == 0
    assert np.array_equal(got[untouched].view(np.uint32), v[untouched].view(np.uint32))       # the bits they went in with
    if n == 63:
        assert untouched.any()
    assert not np.array_equal(got[:, :6], v[:, :6])


def test_nothing_is_skipped():
    rng = np.random.default_rng(5)
    n = 200
    v = random_vertices(rng, n)
    v[7, 0], v[7, 4] = -0.0, -0.0
    targets = random_targets(rng, n, 6, 40)
    targets[2] = (np.array([3, 7, 11], np.uint32), np.array([[np.inf, 1, 1], [1, 2, 3], [1, 1, -np.inf]], np.float32), np.ones((3, 3), np.float32))
    for t in (0, 1, 3, 4, 5):                                                                   # vertices 3, 7 and 11 belong to target 2 alone
        keep = ~np.isin(targets[t][0], (3, 7, 11))
        targets[t] = (targets[t][0][keep], targets[t][1][keep], targets[t][2][keep])
    w = np.array([0.5, -1.0, 0.0, 2.0, 0.25, 1.0], np.float32)                                 # a zero weight on the target with the infinities
    got = glaze_amd.host_morph(v, targets, w)
    assert np.isnan(got[3, 0]) and np.isnan(got[11, 2])                                         # 0 x inf is NaN: the term is not skipped
    assert np.isfinite(got[3, 1:6]).all() and np.isfinite(got[11, [0, 1, 3, 4, 5]]).all()
    assert got[7, 0] == 0.0 and not np.signbit(got[7, 0]) and not np.signbit(got[7, 4])         # -0 + 0 x d is +0
    same_finite_bits(got, restate(v, targets, w, np.float32))
    # NaN and +-inf among the weights and the deltas: the same set of non-finite outputs as the restatement
    targets[0][1][1, 2], targets[4][2][0, 0], targets[5][1][2, 1] = np.nan, np.inf, -np.inf
    for bad in (np.nan, np.inf, -np.inf):
        w2 = w.copy()
        w2[3] = bad
        got = glaze_amd.host_morph(v, targets, w2)
        same_finite_bits(got, restate(v, targets, w2, np.float32))
        assert (~np.isfinite(got)).any() and np.isfinite(got).any()


def test_float32_stays_near_float64():
    rng = np.random.default_rng(11)
    n, n_targets = 3000, 60
    v = random_vertices(rng, n)
    targets = random_targets(rng, n, n_targets, 600, dense=(0, 31))
    w = random_weights(rng, n_targets)
    got = glaze_amd.host_morph(v, targets, w).astype(np.float64)
    exact = restate(v, targets, w, np.float64)
    # A vertex with k terms is a sum of k + 1 addends taken in order.  The addend p passes through the k roundings of the sums; the
    # addend w_i * d_i through the one rounding of its product and at most k roundings of sums: at most k + 1 roundings each, every one
    # of relative size at most U.  So the error is at most ((1 + U)^(k + 1) - 1) L with L = |p| + sum |w_i * d_i|, and
    # (1 + U)^(k + 1) - 1 <= (k + 1) U + ((k + 1) U)^2 <= (k + 2) U as long as (k + 1)^2 U <= 1, which k <= 60 is far inside.
    k = row_lengths(n, targets)[:, None]
    L = np.abs(v[:, :6].astype(np.float64))
    for t, (idx, dp, dn) in enumerate(targets):
        rows = np.arange(n) if idx is None else idx.astype(np.int64)
        L[rows] += np.abs(np.float64(w[t]) * np.concatenate([dp, dn], 1).astype(np.float64))
    assert k.max() >= 20
    assert (np.abs(got[:, :6] - exact[:, :6]) <= (k + 2) * U * L).all()
    assert np.abs(got[:, :6] - exact[:, :6]).max() > 0                                         # (float32 did round somewhere)


def test_composition_with_a_skin_is_skin_of_morph():
    """what the header says an attached morph gives: the morphed vertex is the bind vertex the skinning rule then sees"""
    from test_skin_host import random_bones, random_influences
    from test_skin_host import restate as restate_skin
    rng = np.random.default_rng(21)
    n, n_targets, n_bones = 300, 9, 7
    v, bones = random_vertices(rng, n), random_bones(rng, n_bones)
    j, sw = random_influences(rng, n, n_bones)
    targets, w = random_targets(rng, n, n_targets, 40, dense=(3,)), random_weights(rng, n_targets)
    got = glaze_amd.host_skin(glaze_amd.host_morph(v, targets, w), j, sw, bones)
    same_finite_bits(got, restate_skin(restate(v, targets, w, np.float32), j, sw, bones, np.float32))
    assert not np.array_equal(got[:, :6], glaze_amd.host_skin(v, j, sw, bones)[:, :6])          # the morph did reach the skin


def target_array(entries):
    """(abi.MorphTarget array, what it points into) of (indices or None, d_position or None, d_normal or None, n)"""
    keep = [[None if a is None else np.ascontiguousarray(a, dt) for a, dt in zip(e[:3], (np.uint32, np.float32, np.float32))] for e in entries]
    arr = (abi.MorphTarget * len(entries))(*[abi.MorphTarget(*[None if a is None else a.ctypes.data for a in k], e[3]) for k, e in zip(keep, entries)])
    return arr, keep


def test_refused_arguments():
    lib = abi.lib()
    n = 4
    v = np.zeros((n, 8), np.float32)
    out = np.zeros_like(v)
    d = np.ones((n, 3), np.float32)
    w = np.ones(3, np.float32)
    p = lambda a: a.ctypes.data

    def call(entries, base=v, n_vertices=n, weights=w, result=out, n_targets=None):
        arr, keep = target_array(entries) if entries is not None else (None, None)
        return lib.glz_host_morph(None if base is None else p(base), n_vertices, None if arr is None else C.cast(arr, C.c_void_p),
                                  len(entries) if n_targets is None else n_targets, None if weights is None else p(weights), None if result is None else p(result))

    good = [([0, 2], d[:2], d[:2], 2), (None, d, d, n), (None, None, None, 0)]                    # sparse, dense, and one with n == 0 and null arrays
    assert call(good) == abi.OK
    assert call(good, base=None) == abi.E_ARG and call(good, weights=None) == abi.E_ARG and call(good, result=None) == abi.E_ARG
    assert call(None, n_targets=1) == abi.E_ARG                                                  # null targets
    assert call(good, n_targets=0) == abi.E_ARG and call(good, n_targets=65537) == abi.E_ARG     # n_targets out of 1 .. 65536
    assert call([([0, 4], d[:2], d[:2], 2)]) == abi.E_ARG                                        # an entry index >= n
    assert call([([2, 2], d[:2], d[:2], 2)]) == abi.E_ARG and call([([2, 1], d[:2], d[:2], 2)]) == abi.E_ARG   # not strictly ascending
    assert call([(None, d, d, n - 1)]) == abi.E_ARG and call([(None, d, d, n + 1)]) == abi.E_ARG  # a dense target whose n is not the vertex count
    assert call([([0, 2], None, d[:2], 2)]) == abi.E_ARG and call([([0, 2], d[:2], None, 2)]) == abi.E_ARG     # null deltas where n > 0
    assert call(good, base=None, n_vertices=0, weights=None, result=None) == abi.OK             # no vertices: nothing to read
    assert call(None, base=None, n_vertices=0, weights=None, result=None, n_targets=1) == abi.OK
    assert call(good, result=v) == abi.OK                                                        # out may be base
    with pytest.raises(ValueError):
        glaze_amd.host_morph(v, [(None, d, d)], w)                                              # one weight per target
    with pytest.raises(ValueError):
        glaze_amd.host_morph(v, [(np.array([0, 1]), d, d[:2])], w[:1])


def test_in_place_equals_out_of_place():
    rng = np.random.default_rng(8)
    v = random_vertices(rng, 130)
    targets, w = random_targets(rng, 130, 5, 20, dense=(1,)), random_weights(rng, 5)
    want = glaze_amd.host_morph(v, targets, w)
    arr, keep = glaze_amd._morph_targets(targets, 130)
    assert abi.lib().glz_host_morph(v.ctypes.data, 130, C.cast(arr, C.c_void_p), 5, w.ctypes.data, v.ctypes.data) == abi.OK
    assert np.array_equal(v.view(np.uint32), want.view(np.uint32))


def test_the_header_states_the_rule():
    text = open(os.path.join(ROOT, "include", "glaze_abi.h"), encoding="utf-8").read()
    for piece in ("THE MORPH RULE", "p' = ((…((p + w[t1] * dp_1) + w[t2] * dp_2) …) + w[tk] * dp_k)",
                  "n' = ((…((n + w[t1] * dn_1) + w[t2] * dn_2) …) + w[tk] * dn_k)", "t' = t", "glz_host_skin(glz_host_morph(bind, ...), ...)"):
        assert piece in text, piece


def test_the_python_constant_is_the_kernels():
    text = open(os.path.join(ROOT, "glaze_amd", "csrc", "kernels.h")).read()
    assert int(re.search(r"kMorphLdsTargets = (\d+);", text).group(1)) == abi.MORPH_LDS_TARGETS
