"""The clip rule on the host (glz_host_clip_bones: the reference k_clip_bones must match bit for bit) against the specification in
include/glaze_abi.h ("THE CLIP RULE"), restated in numpy float32 with one operation per numpy call in the specification's order
(tests/clip_cases.py; bit for bit), and against mathematics on cases whose every value is exactly representable.  No device."""
import ctypes as C
import os

import numpy as np
import pytest

import glaze_amd
from glaze_amd import abi

import clip_cases as cc

F = np.float32
IDENT = np.eye(4, dtype=F).reshape(16)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def same_bits(a, b):
    """bit for bit, except that any NaN equals any NaN (the payload is the hardware's)"""
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return a.shape == b.shape and bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))


def identity_binds(n):
    return np.tile(IDENT, (n, 1))


def unit_rotations(n_keys, n_bones):
    return np.tile(np.array([0, 0, 0, 1], F), (n_keys, n_bones, 1))


SKELETONS = [("one", 1, lambda rng: cc.chain(1)), ("two", 2, lambda rng: cc.chain(2)), ("tree7", 7, lambda rng: cc.random_tree(rng, 7, roots=2)),
             ("tree300", 300, lambda rng: cc.random_tree(rng, 300)), ("chain300", 300, lambda rng: cc.chain(300))]


@pytest.mark.parametrize("name,n_bones,make", SKELETONS, ids=[s[0] for s in SKELETONS])
@pytest.mark.parametrize("n_keys", [1, 2, 5])
def test_host_matches_the_restated_rule_bit_for_bit(name, n_bones, make, n_keys):
    rng = np.random.default_rng(1000 * n_bones + n_keys)
    parents = make(rng)
    ib, root = cc.random_rigid(rng, n_bones), cc.random_rigid(rng, 1)[0]
    for scaled, n_targets in ((True, 3), (False, 0)):
        times, tr, ro, sc, mw = cc.random_clip(rng, n_bones, n_keys, scaled, n_targets)
        for t in cc.times_around(times):
            got = glaze_amd.host_clip_bones(parents, ib, times, tr, ro, t, scales=sc, morph_weights=mw, root=root)
            want, want_w = cc.restate(parents, ib, times, tr, ro, t, scales=sc, morph_weights=mw, root=root)
            bones, weights = got if n_targets else (got, None)
            assert np.isfinite(bones).all()
            assert same_bits(bones, want), (name, n_keys, float(t))
            assert np.array_equal(bones[:, [3, 7, 11, 15]], np.tile(np.array([0, 0, 0, 1], F), (n_bones, 1)))
            if n_targets:
                assert same_bits(weights, want_w)


def test_exact_three_deep_chain_against_matrices_written_out_by_hand():
    # identity rotations, integer translations, power-of-two scales, u in {0, 1/4, 1/2}: every value is exact in float32
    parents = cc.chain(3)
    times = np.array([0, 4], F)
    tr = np.array([[[1, 2, 3], [4, 0, 0], [0, 8, 0]], [[5, 2, 3], [4, 8, 0], [0, 8, 16]]], F)
    sc = np.array([[[2, 2, 2], [1, 1, 1], [0.5, 0.5, 0.5]], [[2, 2, 2], [1, 1, 1], [0.5, 0.5, 0.5]]], F)
    ro = unit_rotations(2, 3)
    ib = identity_binds(3)
    ib[1, 12:15] = [-1, -2, -3]   # a translation by (-1, -2, -3)

    def expected(u):
        # locals: L0 = T(1 + 4u, 2, 3) S(2);  L1 = T(4, 8u, 0);  L2 = T(0, 8, 16u) S(1/2)
        # W0 = L0;  W1 = W0 L1 = [2 I | (1 + 4u, 2, 3) + 2 (4, 8u, 0)];  W2 = W1 L2 = [I | W1.t + 2 (0, 8, 16u)]
        w0 = (1 + 4 * u, 2, 3)
        w1 = (w0[0] + 8, w0[1] + 16 * u, w0[2])
        w2 = (w1[0], w1[1] + 16, w1[2] + 32 * u)
        b1 = (w1[0] + 2 * -1, w1[1] + 2 * -2, w1[2] + 2 * -3)   # W1 o T(-1, -2, -3)
        return [[2, 0, 0, 0, 0, 2, 0, 0, 0, 0, 2, 0, w0[0], w0[1], w0[2], 1], [2, 0, 0, 0, 0, 2, 0, 0, 0, 0, 2, 0, b1[0], b1[1], b1[2], 1],
                [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, w2[0], w2[1], w2[2], 1]]

    for t, u in ((0.0, 0.0), (1.0, 0.25), (2.0, 0.5)):
        got = glaze_amd.host_clip_bones(parents, ib, times, tr, ro, t, scales=sc)
        assert np.array_equal(got, np.array(expected(u), F)), t
    # under a root that doubles and moves: every matrix is root o the one above
    root = np.array([2, 0, 0, 0, 0, 2, 0, 0, 0, 0, 2, 0, 16, 32, 64, 1], F)
    got = glaze_amd.host_clip_bones(parents, ib, times, tr, ro, 2.0, scales=sc, root=root)
    want = np.array(expected(0.5), F)
    want[:, [0, 5, 10]] *= 2
    want[:, 12:15] = want[:, 12:15] * 2 + np.array([16, 32, 64], F)
    assert np.array_equal(got, want)


def test_key_choice_on_a_key_takes_it_with_u_zero():
    rng = np.random.default_rng(7)
    parents, ib = cc.random_tree(rng, 7, roots=2), cc.random_rigid(rng, 7)
    times, tr, ro, sc, _ = cc.random_clip(rng, 7, 5)
    for k in range(5):
        on_key = glaze_amd.host_clip_bones(parents, ib, times, tr, ro, times[k], scales=sc)
        alone = glaze_amd.host_clip_bones(parents, ib, times[k:k + 1], tr[k:k + 1], ro[k:k + 1], 0.0, scales=sc[k:k + 1])
        assert same_bits(on_key, alone), k
    # and the restated choice says so itself
    assert cc.key_choice(times, times[2]) == (2, 3, F(0)) and cc.key_choice(times, times[4]) == (4, 4, F(0)) and cc.key_choice(times, times[0]) == (0, 0, F(0))


def test_equal_keys_return_finite_values_unchanged():
    # k0 == k1 (one key): translation, scale and weights come back as they are; the rotation is only normalised
    parents, ib = cc.chain(1), identity_binds(1)
    tr = np.array([[[0.1, -7.3, 1e-30]]], F)
    sc = np.array([[[3.7, 0.3, 1e10]]], F)
    mw = np.array([[0.123, -4.5e-20, 7e15]], F)
    bones, w = glaze_amd.host_clip_bones(parents, ib, [5.0], tr, unit_rotations(1, 1), 99.0, scales=sc, morph_weights=mw)
    assert same_bits(bones[0, 12:15], tr[0, 0]) and same_bits(bones[0, [0, 5, 10]], sc[0, 0]) and same_bits(w, mw[0])


def test_hemisphere_step():
    rng = np.random.default_rng(11)
    parents, ib = cc.random_tree(rng, 7), cc.random_rigid(rng, 7)
    times, tr, ro, sc, _ = cc.random_clip(rng, 7, 2)
    ro[1] = ro[0]
    same = glaze_amd.host_clip_bones(parents, ib, times, tr, ro, times[0] + F(0.25) * (times[1] - times[0]), scales=sc)
    ro[1] = -ro[0]   # the same rotation on the other hemisphere: dot < 0, b enters negated and IS a
    flipped = glaze_amd.host_clip_bones(parents, ib, times, tr, ro, times[0] + F(0.25) * (times[1] - times[0]), scales=sc)
    assert same_bits(same, flipped)
    # A dot of -0 keeps b.  a = (1, 0, 0, 0), b = (-0, -1, -1, -1): every product is -0, so dot = ((-0 + -0) + -0) + -0 = -0.  Kept:
    # Q = a + 0.5 * (b - a) = (1/2, -1/2, -1/2, -1/2), unit already, so q = Q and the matrix below, exactly.  Negated, b would be
    # (0, 1, 1, 1) and Q = (1/2, 1/2, 1/2, 1/2): another rotation.
    a, b = np.array([1, 0, 0, 0], F), np.array([-0.0, -1, -1, -1], F)
    args = (cc.chain(1), identity_binds(1), [0.0, 1.0], np.zeros((2, 1, 3), F), np.stack([a, b]).reshape(2, 1, 4), 0.5)
    got = glaze_amd.host_clip_bones(*args)
    assert same_bits(got, cc.restate(*args)[0])
    assert np.array_equal(got[0], np.array([0, 0, -1, 0, -1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 1], F))
    # a NaN dot keeps b too: the NaN goes through the lerp and the normalisation, and nothing is skipped
    args = (cc.chain(1), identity_binds(1), [0.0, 1.0], np.zeros((2, 1, 3), F), np.stack([a, np.array([np.nan, 0, 0, 1], F)]).reshape(2, 1, 4), 0.5)
    got = glaze_amd.host_clip_bones(*args)
    assert same_bits(got, cc.restate(*args)[0]) and np.isnan(got[0, [0, 1, 2, 4, 5, 6, 8, 9, 10]]).all()


def test_non_finite_keys_reach_the_output_as_the_rule_says():
    parents, ib = cc.chain(2), identity_binds(2)
    tr = np.zeros((2, 2, 3), F)
    tr[0, 0, 0] = np.inf    # lerp at u = 0: inf + 0 * (0 - inf) = inf + nan = NaN -- the term is not skipped
    tr[1, 1, 1] = np.nan
    ro = unit_rotations(2, 2)
    for t in (0.0, 0.5, 1.0, -3.0):
        args = (parents, ib, [0.0, 1.0], tr, ro, t)
        got, want = glaze_amd.host_clip_bones(*args), cc.restate(*args)[0]
        assert same_bits(got, want)
        if t < 1.0:   # key 0 takes part: bone 0's x, and its child's through the hierarchy
            assert np.isnan(got[0, 12]) and np.isnan(got[1, 12])
        if t == 1.0:   # key 1 alone: bone 1's y, and nothing of its parent
            assert np.isnan(got[1, 13]) and np.isfinite(got[0]).all()
    one_key = glaze_amd.host_clip_bones(cc.chain(1), identity_binds(1), [0.0], np.array([[[np.inf, 1, 2]]], F), unit_rotations(1, 1), 0.0)
    # k0 == k1: an infinity becomes NaN (inf + 0 * (inf - inf)), and root o L spreads it over the column (0 * NaN is NaN); the 3 x 3 is clean
    assert np.isnan(one_key[0, 12:15]).all() and np.array_equal(one_key[0, :12], IDENT[:12])
    # a zero rotation is not special-cased: 1 / sqrt(0) is inf, 0 * inf is NaN
    zero = glaze_amd.host_clip_bones(cc.chain(1), identity_binds(1), [0.0], np.zeros((1, 1, 3), F), np.zeros((1, 1, 4), F), 0.0)
    assert np.isnan(zero[0, [0, 1, 2, 4, 5, 6, 8, 9, 10]]).all()


def test_weight_track_is_lerped_per_target():
    parents, ib = cc.chain(1), identity_binds(1)
    mw = np.array([[0, 8, -4, 1], [4, 8, 4, 3], [4, 0, 0, 3]], F)
    args = (parents, ib, [0.0, 4.0, 8.0], np.zeros((3, 1, 3), F), unit_rotations(3, 1))
    for t, want in ((1.0, [1, 8, -2, 1.5]), (2.0, [2, 8, 0, 2]), (6.0, [4, 4, 2, 3]), (-1.0, [0, 8, -4, 1]), (9.0, [4, 0, 0, 3]), (4.0, [4, 8, 4, 3])):
        _, w = glaze_amd.host_clip_bones(*args, t, morph_weights=mw)
        assert np.array_equal(w, np.array(want, F)), t


def _call(sk, clip, time, bones, weights=None):
    return abi.lib().glz_host_clip_bones(None if sk is None else C.cast(C.byref(sk), C.c_void_p), None if clip is None else C.cast(C.byref(clip), C.c_void_p),
                                         C.c_float(time), None if bones is None else bones.ctypes.data, None if weights is None else weights.ctypes.data)


def test_refusals():
    n = 3
    parents, ib = cc.chain(n), identity_binds(n)
    times, tr, ro = np.array([0, 1], F), np.zeros((2, n, 3), F), unit_rotations(2, n)
    bones = np.zeros((n, 16), F)
    ptr = lambda a: a.ctypes.data

    def skeleton(p=parents, n_bones=n, with_parents=True, with_ib=True):
        p = np.ascontiguousarray(p, np.int32)
        keep.append(p)
        return abi.Skeleton(-1, n_bones, ptr(p) if with_parents else None, ptr(ib) if with_ib else None, (C.c_float * 16)(*IDENT))

    def clip(t=times, n_keys=2, **null):
        t = np.ascontiguousarray(t, F)
        keep.append(t)
        return abi.Clip(-1, n_keys, None if null.get("times") else ptr(t), None if null.get("translations") else ptr(tr), None if null.get("rotations") else ptr(ro), None, None, 0)

    keep = []
    assert _call(skeleton(), clip(), 0.5, bones) == abi.OK
    bad = [(None, clip(), 0.5, bones), (skeleton(), None, 0.5, bones), (skeleton(), clip(), 0.5, None), (skeleton(with_parents=False), clip(), 0.5, bones),
           (skeleton(with_ib=False), clip(), 0.5, bones), (skeleton(), clip(times=True), 0.5, bones), (skeleton(), clip(translations=True), 0.5, bones),
           (skeleton(), clip(rotations=True), 0.5, bones), (skeleton(n_bones=0), clip(), 0.5, bones), (skeleton(), clip(n_keys=0), 0.5, bones),
           (skeleton(), clip(t=[1, 1]), 0.5, bones), (skeleton(), clip(t=[1, 0]), 0.5, bones), (skeleton(), clip(t=[0, np.nan]), 0.5, bones),
           (skeleton(), clip(t=[0, np.inf]), 0.5, bones), (skeleton(p=[-1, 1, 0]), clip(), 0.5, bones), (skeleton(p=[-1, 2, 0]), clip(), 0.5, bones),
           (skeleton(p=[0, 0, 0]), clip(), 0.5, bones), (skeleton(p=[-1, -2, 0]), clip(), 0.5, bones), (skeleton(), clip(), np.nan, bones),
           (skeleton(), clip(), np.inf, bones)]
    before = bones.copy()
    for i, args in enumerate(bad):
        assert _call(*args) == abi.E_ARG, i
    assert np.array_equal(bones, before)


def test_the_header_states_the_rule():
    text = open(os.path.join(ROOT, "include", "glaze_abi.h"), encoding="utf-8").read()
    for phrase in ("THE CLIP RULE", "lerp(a, b) = a + u * (b - a)", "b enters negated if dot < 0", "nn == 0 is NOT special-cased", "never\n *        regrouped"):
        assert phrase in text, phrase
