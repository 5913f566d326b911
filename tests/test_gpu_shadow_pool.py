"""k_trace's pool of shadow groups (glaze_amd/csrc/device/trace_split.h, kernels_render.hip): part of a launch's shadow groups stays
undealt and is drawn, chunk by chunk, by whichever wave finishes its fixed share first.

Which wave traces a shadow ray, and when within the kernel, may change nothing: every shadow ray belongs to one pixel and a pixel has at
most one per launch.  So whole renders are compared with the oracle bit for bit, for the settings that take the kernel's different
ways: pool off (the division before there was a pool), the default, a quarter in the pool, everything in the pool, chunks of one group, one chunk larger than
the pool.  The waves only specialise with more 64-ray groups than waves: GLAZE_TRACE_BLOCKS_PER_CU=1 leaves 1 024 waves, and a 256 x 256
frame has 1 024 closest-hit groups plus its shadow groups.  The scene is the small atrium: a closed courtyard lit by sun and sky, whose
shadow rays end both ways (test_gpu_shadow_order.test_any_hit_parity: neither all occluded nor all free).
"""
import numpy as np
import pytest

import glaze_amd
from glaze_amd.scenes import atrium_scene
from oracle.pyoracle import OracleRenderer, OracleScene

pytestmark = pytest.mark.gpu

DEPTH, SEED, LAUNCHES = 4, 7, 12
SETTINGS = {
    "pool_off": "8/10,0/1,1",
    "default": None,                 # device/tuning.h: the pool is off there too, at another static share
    "pool_quarter": "7/10,1/4,2",
    "pool_share_1": "7/10,1/1,2",
    "chunk_1": "7/10,1/4,1",
    "chunk_larger_than_pool": "7/10,1/4,60000",
}


def bits(a):
    return np.nan_to_num(a, nan=-1.0).view(np.uint32)


def oracle_frame(desc, w, h):
    o = OracleRenderer(OracleScene(desc), w, h)
    o.set_depth(DEPTH)
    o.set_seed(SEED)
    o.step(LAUNCHES)
    return o.read_hdr()


@pytest.fixture(scope="module")
def atrium():
    desc = atrium_scene(detail=0.05, texture_size=64, sky_size=(256, 128))
    return desc, oracle_frame(desc, 256, 256)


def renderer(instance, monkeypatch, desc, w, h, setting, capped=True):
    """the environment is read when the renderer is created"""
    if capped:
        monkeypatch.setenv("GLAZE_TRACE_BLOCKS_PER_CU", "1")
    else:
        monkeypatch.delenv("GLAZE_TRACE_BLOCKS_PER_CU", raising=False)
    if setting is None:
        monkeypatch.delenv("GLAZE_TRACE_SPLIT", raising=False)
    else:
        monkeypatch.setenv("GLAZE_TRACE_SPLIT", setting)
    r = glaze_amd.RayTraceRenderer.new(instance, glaze_amd.RayTraceScene.from_desc(instance, desc), w, h)
    r.set_launch_mode("two_kernels")
    r.set_depth(DEPTH)
    r.set_seed(SEED)
    return r


def same(got, want):
    assert np.array_equal(bits(got), bits(want)), "%d pixels differ" % (bits(got) != bits(want)).any(-1).sum()
    assert (got[..., :3].sum(-1) > 0).mean() > 0.5


@pytest.mark.parametrize("which", list(SETTINGS))
def test_render_equals_the_oracle(instance, monkeypatch, atrium, which):
    desc, want = atrium
    r = renderer(instance, monkeypatch, desc, 256, 256, SETTINGS[which])
    r.step(LAUNCHES)
    same(r.read_hdr(), want)


def test_no_split_without_the_cap(instance, monkeypatch):
    """128 x 128 on the whole chip: fewer groups than waves, every group has a wave of its own and nothing is drawn"""
    desc = atrium_scene(detail=0.05, texture_size=64, sky_size=(256, 128))
    r = renderer(instance, monkeypatch, desc, 128, 128, None, capped=False)
    r.step(LAUNCHES)
    same(r.read_hdr(), oracle_frame(desc, 128, 128))


def test_frame_read_after_every_launch(instance, monkeypatch, atrium):
    """a read drains the queued shadow rays in a stand-alone pass, which neither splits nor draws, between launches that use the two
    pool heads alternately"""
    desc, want = atrium
    r = renderer(instance, monkeypatch, desc, 256, 256, "7/10,1/4,2")
    for _ in range(LAUNCHES):
        r.step(1)
        got = r.read_hdr()
    same(got, want)


def test_restart_in_the_middle(instance, monkeypatch, atrium):
    """a restart drops the queued shadow rays and clears both heads: the frame after it is the frame of a fresh renderer"""
    desc, want = atrium
    r = renderer(instance, monkeypatch, desc, 256, 256, "7/10,1/2,1")
    r.step(5)
    r.restart()
    r.step(LAUNCHES)
    same(r.read_hdr(), want)


def test_scene_with_opacity_maps(instance, monkeypatch):
    """k_trace<false, kAlphaPhase>: the other product instantiation"""
    desc = atrium_scene(sponza_like=True, texture_size=64, sky_size=(64, 32))
    r = renderer(instance, monkeypatch, desc, 256, 256, "7/10,1/4,2")
    r.step(LAUNCHES)
    same(r.read_hdr(), oracle_frame(desc, 256, 256))
