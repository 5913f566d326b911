"""The host references of the motion / reprojection specification (include/glaze_abi.h, above glz_reproject_params) against a float64
restatement of that comment (tests/reproject_ref.py): glz_host_project_constants, glz_host_project_points, glz_host_reproject.  No device.
The device kernels are compared with these references bit for bit in tests/test_gpu_motion.py."""
import ctypes as C

import numpy as np
import pytest

import glaze_amd
from glaze_amd import abi

from denoise_ref import synthetic_frame
from reproject_ref import (REPROJECT_CASES, accepted_taps, bits, cameras, projection_bounds, projection_points, reference_project, reference_reproject,
                           reproject_inputs)


# ---------------------------------------------------------------------------------------------------------------------
# 1. host_project_points against float64
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cameras()))
def test_host_project_points_against_float64(name):
    cam = cameras()[name]
    w, h = 128, 72
    persp = cam.type == abi.CAMERA_PERSPECTIVE
    w2c, c2s = glaze_amd.host_project_constants(cam, w, h)
    pts = projection_points(cam, 4096, seed=11)
    got = glaze_amd.host_project_points(cam, w, h, pts)
    want, valid, z_c = reference_project(w2c, c2s, persp, w, h, pts)
    got_valid = np.isfinite(got[:, 2])
    assert np.array_equal(got_valid, valid), "the invalid sets differ at %s" % np.argwhere(got_valid != valid)[:4].ravel()
    assert valid.sum() > 1000 and (~valid).sum() >= 10
    assert (got[~valid, :2] == 0).all() and np.isposinf(got[~valid, 2]).all()
    bx, by, bz = projection_bounds(c2s, persp, w, h, pts[valid], cam.position[:], z_c[valid], want[valid, 2])
    ex, ey = np.abs(got[valid, 0] - want[valid, 0]), np.abs(got[valid, 1] - want[valid, 1])
    ez = np.abs(got[valid, 2] - want[valid, 2]) / want[valid, 2]
    print("%s: %d valid points, largest error / bound: fx %.3f, fy %.3f, z %.3f" % (name, valid.sum(), (ex / bx).max(), (ey / by).max(), (ez / bz).max()))
    assert (ex <= bx).all() and (ey <= by).all() and (ez <= bz).all()


# ---------------------------------------------------------------------------------------------------------------------
# 2. host_project_constants: the forward twins of the push constants
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cameras()))
def test_project_constants_invert_the_push_constants(name):
    cam = cameras()[name]
    for w, h in ((128, 72), (97, 61)):
        w2c, c2s = glaze_amd.host_project_constants(cam, w, h)
        push = np.zeros(32, np.float32)
        abi.check(abi.lib().glz_host_push_constants(C.byref(cam), w, h, push.ctypes.data))
        for forward, inverse in ((w2c, push[:16]), (c2s, push[16:])):
            a, b = forward.astype(np.float64).reshape(4, 4).T, inverse.astype(np.float64).reshape(4, 4).T
            # each entry of both is a binary32 rounding (2^-24 relative): the product's entries move by that much of the products summed
            assert (np.abs(a @ b - np.eye(4)) <= 1e-6 * (np.abs(a) @ np.abs(b))).all(), (name, w, h)
    with pytest.raises(glaze_amd.GlazeError) as e:
        glaze_amd.host_project_constants(cam, 0, 72)
    assert e.value.status == -4


# ---------------------------------------------------------------------------------------------------------------------
# 3. host_reproject against the float64 restatement fed the same float32 inputs
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size,shift", REPROJECT_CASES)
def test_host_reproject_against_float64(size, shift):
    motion, color, aov0, aov1 = reproject_inputs(size[0], size[1], seed=size[0] + int(4 * shift[0]), shift=shift)
    want, taps, edge = reference_reproject(motion, color, aov0, aov1)
    print("%dx%d shift %s: %d of %d pixels sit on a decision (cap %d)" % (size[0], size[1], shift, edge.sum(), edge.size, int(0.005 * edge.size)))
    assert edge.sum() <= 0.005 * edge.size                                  # a condition on the inputs, not a measurement
    got = glaze_amd.host_reproject(motion, color, aov0, aov1)
    got_taps = accepted_taps(glaze_amd.host_reproject, motion, color, aov0, aov1)
    keep = ~edge
    n_taps = taps[keep].sum(-1)
    assert (n_taps == 4).sum() > 0.2 * keep.sum() and ((n_taps > 0) & (n_taps < 4)).sum() > 0.02 * keep.sum() and (n_taps == 0).sum() > 0.05 * keep.sum(), np.bincount(n_taps)
    differ = (got_taps != taps).any(-1) & keep
    assert not differ.any(), "%d pixels accept other taps, first at %s" % (differ.sum(), np.argwhere(differ)[0])
    none = keep & ~taps.any(-1)
    assert (bits(got[none]) == 0).all()
    some = keep & taps.any(-1)
    err = np.abs(got[some].astype(np.float64) - want[some]) / np.maximum(np.abs(want[some]), 1e-30)
    print("  largest relative error %.3g" % err.max())
    assert err.max() <= 1e-5


# ---------------------------------------------------------------------------------------------------------------------
# 4. exact properties
# ---------------------------------------------------------------------------------------------------------------------
def test_zero_motion_returns_the_frame_bit_for_bit():
    color, aov0, aov1, region = synthetic_frame(150, 83, seed=5)
    motion = np.zeros_like(color)
    motion[..., 2] = aov0[..., 3]
    motion[..., 3] = aov1[..., 3]
    out = glaze_amd.host_reproject(motion, color, aov0, aov1)
    hit = region > 0
    assert np.array_equal(bits(out[hit][:, :3]), bits(color[hit][:, :3])) and (out[hit][:, 3] == 1.0).all()
    assert (bits(out[~hit]) == 0).all()


def test_other_instances_do_not_reach_a_pixel():
    motion, color, aov0, aov1 = reproject_inputs(150, 83, seed=9, shift=(1.5, -0.5))
    out = glaze_amd.host_reproject(motion, color, aov0, aov1)
    ids = bits(aov1[..., 3])
    for inst in (0, 1):
        scaled = color.copy()
        scaled[ids != inst] *= np.float32(7.0)
        again = glaze_amd.host_reproject(motion, scaled, aov0, aov1)
        mine = bits(motion[..., 3]) == inst
        assert mine.sum() > 1000 and np.array_equal(bits(again[mine]), bits(out[mine]))


def test_invalid_tolerances_are_argument_errors():
    motion, color, aov0, aov1 = reproject_inputs(40, 30, seed=2, shift=(0.5, 0.5))
    for bad in (0.0, -1.0, np.nan, np.inf, -np.inf):
        with pytest.raises(glaze_amd.GlazeError) as e:
            glaze_amd.host_reproject(motion, color, aov0, aov1, depth_tolerance=bad)
        assert e.value.status == -4, bad
    assert glaze_amd.host_reproject(motion, color, aov0, aov1, depth_tolerance=1e-3).shape == motion.shape
