"""The texture sampler against a float64 reference (tests/texref.py) and, on the device, against the oracle bit for bit.

The sampler (device/shading.h bilinear_level / texture2d_lod, restated by oracle.cpp texture_bilinear_level / texture_lod) is reached
by every diffuse, roughness, metalness, normal and opacity fetch; renders only ever give it small coordinates.  Here it runs on its
own, through glz_debug_sample_texture / orc_sample_texture, at the sizes where the tiled layout and the wrap go wrong (1 x 1 inline
texel, single rows and columns, exact tiles, one texel past a tile, a large texture behind others in the pool) and at the coordinates
where float32 texel indices go wrong (|u w| across 2^22 .. 2^32, 1e20, FLT_MAX, inf, NaN)."""
import ctypes as C

import numpy as np
import pytest

import glaze_amd
from glaze_amd import abi
from glaze_amd.scene_desc import INSTANCE_DTYPE, MESH_DTYPE, VERTEX_DTYPE, SceneDesc, make_camera, make_light, make_material, make_meta
from oracle.pyoracle import OracleRenderer, OracleScene

import texref

F32_MAX = float(np.finfo(np.float32).max)

# (width, height, format): the inline 1 x 1 texel, a row, a column, ragged tiles, exact tiles (8 x 4 RGBA, 16 x 8 gray), one texel
# past a tile, a larger one, and every sRGB code in one row
SIZES = [(1, 1, abi.TEX_RGBA_SRGB), (1, 1, abi.TEX_GRAY), (1, 7, abi.TEX_RGBA_NORM), (5, 1, abi.TEX_RGBA_SRGB), (7, 3, abi.TEX_GRAY),
         (7, 3, abi.TEX_RGBA_SRGB), (8, 4, abi.TEX_RGBA_NORM), (8, 4, abi.TEX_RGBA_SRGB), (16, 8, abi.TEX_GRAY), (9, 5, abi.TEX_RGBA_SRGB),
         (17, 9, abi.TEX_GRAY), (130, 66, abi.TEX_RGBA_NORM), (130, 66, abi.TEX_GRAY)]
SRGB_ROW = len(SIZES) + 1          # texture id of the 256 x 1 row of every sRGB code (id 0 is the default white texel)


def texture_pixels(w, h, fmt, seed):
    rng = np.random.default_rng(seed)
    if fmt == abi.TEX_GRAY:
        return rng.integers(0, 256, (h, w), dtype=np.uint8)
    px = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    return px


def srgb_row():
    c = np.arange(256, dtype=np.uint8)
    return np.stack([c, c[::-1], c, c[::-1]], -1)[None]


def textured_desc(textures):
    """one triangle; `textures` = [(format, pixels)], after the 1 x 1 white default"""
    vertices = np.zeros(3, VERTEX_DTYPE)
    for i, q in enumerate([(0, 0, 1), (1, 0, 1), (0, 1, 1)]):
        vertices[i] = (q, (0.0, 0.0, -1.0), q[:2])
    texs = [(abi.TEX_RGBA_SRGB, np.full((1, 1, 4), 255, np.uint8), "default")]
    texs += [(fmt, px, "t%d" % i) for i, (fmt, px) in enumerate(textures)]
    return SceneDesc(vertices, np.array([0, 1, 2], np.uint32), np.array([(0, 0, 0, 3)], MESH_DTYPE), None, np.array([(0, 0)], INSTANCE_DTYPE),
                     [make_material("default")], [make_light(abi.LIGHT_SUN, "sun", direction=(0.0, 0.0, 1.0))], texs, make_camera(), make_meta())


def sampler_desc():
    return textured_desc([(fmt, texture_pixels(w, h, fmt, 17 + i)) for i, (w, h, fmt) in enumerate(SIZES)] + [(abi.TEX_RGBA_SRGB, srgb_row())])


def crossings(size):
    """u where |u * size| crosses 2^22, 2^23, 2^24, 2^31, 2^32, from both sides and with both signs"""
    out = []
    for p in (22, 23, 24, 31, 32):
        c = np.float32(2.0 ** p / size)
        x = c
        for _ in range(3):
            x = np.nextafter(x, np.float32(0))
        y = x
        for _ in range(7):
            out += [y, -y]
            y = np.nextafter(y, np.float32(np.inf))
        out += [c * np.float32(1.5), -c * np.float32(1.5), c + np.float32(0.25) / size]
    return np.array(out, np.float32)


SPECIAL = np.array([0.0, -0.0, 1e-45, -1e-45, 1.1754942e-38, -1e-39, 1e20, -1e20, 3e9, -3e9, F32_MAX, -F32_MAX, np.inf, -np.inf, np.nan],
                   np.float32)


def coordinates(w, h, seed, huge_only=False):
    """(u, v) float32 arrays: texel centres and edges, random values in [0, 1) and [-4, 4], the special values, the crossings"""
    rng = np.random.default_rng(seed)
    cu, cv = crossings(w), crossings(h)
    far_u = np.concatenate([cu[np.abs(cu.astype(np.float64) * w) >= 2 ** 22], SPECIAL[6:]])
    far_v = np.concatenate([cv[np.abs(cv.astype(np.float64) * h) >= 2 ** 22], SPECIAL[6:]])
    us, vs = [], []

    def add(u, v):
        u, v = np.broadcast_arrays(np.asarray(u, np.float32), np.asarray(v, np.float32))
        us.append(u.ravel())
        vs.append(v.ravel())

    if huge_only:
        add(far_u[:, None], rng.uniform(0, 1, (1, 8)))
        add(rng.uniform(-4, 4, (8, 1)), far_v[None, :])
        add(far_u[:, None], far_v[None, :])
        return np.concatenate(us), np.concatenate(vs)
    iu, iv = np.arange(min(w, 40)), np.arange(min(h, 40))
    add(((iu + 0.5) / w)[:, None], ((iv + 0.5) / h)[None, :])             # centres
    add((iu / w)[:, None], (iv / h)[None, :])                               # edges
    add(((iu + 0.5) / w - 3)[:, None], ((iv + 0.5) / h + 2)[None, :])       # centres of other periods
    add(rng.uniform(0, 1, 3000), rng.uniform(0, 1, 3000))
    add(rng.uniform(-4, 4, 3000), rng.uniform(-4, 4, 3000))
    add(SPECIAL[:, None], SPECIAL[None, :])
    add(SPECIAL[:, None], rng.uniform(-4, 4, (1, 4)))
    add(rng.uniform(-4, 4, (4, 1)), SPECIAL[None, :])
    add(cu[:, None], rng.uniform(0, 1, (1, 4)))
    add(rng.uniform(0, 1, (4, 1)), cv[None, :])
    add(cu[:, None], cv[None, ::5])
    return np.concatenate(us), np.concatenate(vs)


def check_against_reference(got, px, fmt, u, v, what):
    tex = texref.decode(fmt, px if px.ndim == 3 or fmt == abi.TEX_GRAY else px)
    h, w = tex.shape[:2]
    want, lo, hi = texref.bilinear(tex, u, v)
    nan_want = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan_want), "%s: NaN results differ from the reference at %s" % (
        what, list(zip(u[(np.isnan(got) != nan_want).any(1)][:4], v[(np.isnan(got) != nan_want).any(1)][:4])))
    ok = ~nan_want.any(1)
    bound = texref.level0_bound(want, lo, hi, u, w, v, h)
    err = np.abs(got[ok].astype(np.float64) - want[ok])
    bad = (err > bound[ok]).any(1)
    assert not bad.any(), "%s: %d fetches off the float64 reference, e.g. uv %s got %s want %s" % (
        what, bad.sum(), (u[ok][bad][0], v[ok][bad][0]), got[ok][bad][0], want[ok][bad][0])
    # a bilinear blend never leaves the range of the four texels it blends (as float32 values)
    lo32, hi32 = lo[ok].astype(np.float32), hi[ok].astype(np.float32)
    out = (got[ok] < lo32) | (got[ok] > hi32)
    assert not out.any(), "%s: %d fetches outside their texels' range, e.g. uv %s" % (what, out.any(1).sum(), (u[ok][out.any(1)][0], v[ok][out.any(1)][0]))
    # exactly the texel where the float32 sample point is a texel centre (|u w| < 2^22)
    fu, fv = texref.sample_point(u, w), texref.sample_point(v, h)
    cen = ok & (fu == np.floor(fu)) & (fv == np.floor(fv)) & (np.abs(fu) < 2 ** 22) & (np.abs(fv) < 2 ** 22)
    assert np.array_equal(got[cen], want[cen].astype(np.float32)), what + ": a texel centre is not exactly its texel"


@pytest.fixture(scope="module")
def oracle_sampler():
    desc = sampler_desc()
    return desc, OracleScene(desc)


@pytest.mark.parametrize("k", range(len(SIZES)))
def test_oracle_sampler_matches_float64_reference(oracle_sampler, k):
    desc, sc = oracle_sampler
    w, h, fmt = SIZES[k]
    px = desc.textures[k + 1][1]
    u, v = coordinates(w, h, k)
    check_against_reference(sc.sample_texture(k + 1, np.stack([u, v], -1)), px, fmt, u, v, "oracle %dx%d fmt %d" % (w, h, fmt))


@pytest.mark.parametrize("k", range(len(SIZES)))
def test_oracle_sampler_huge_coordinates(oracle_sampler, k):
    """|u w| or |v h| >= 2^22 up to FLT_MAX, inf and NaN: the texel index wraps exactly and the weight is that of the float32 sample
    point (0 from 2^23 on).  A float -> int conversion out of range (the texel index of 2^31 and beyond, or glz_floorf's own) gives
    weights of about 1e9 and results far outside the texels."""
    desc, sc = oracle_sampler
    w, h, fmt = SIZES[k]
    u, v = coordinates(w, h, k, huge_only=True)
    check_against_reference(sc.sample_texture(k + 1, np.stack([u, v], -1)), desc.textures[k + 1][1], fmt, u, v, "oracle huge %dx%d" % (w, h))


def test_oracle_srgb_row_is_the_eotf():
    """texel centres of the 256 x 1 row of every code: float32(EOTF(code / 255)) exactly (no table built by either side)"""
    sc = OracleScene(sampler_desc())
    u = (np.arange(256, dtype=np.float32) + np.float32(0.5)) / np.float32(256)
    got = sc.sample_texture(SRGB_ROW, np.stack([u, np.full(256, 0.5, np.float32)], -1))
    code = np.arange(256)
    want = np.stack([texref.eotf(code / 255.0), texref.eotf(code[::-1] / 255.0), texref.eotf(code / 255.0), code[::-1] / 255.0], -1)
    assert np.array_equal(got, want.astype(np.float32))


# ---- texture level of detail --------------------------------------------------------------------------------------------------
LOD_TEXTURES = [k for k, (w, h, _) in enumerate(SIZES) if w * h > 1]


def host_levels(fmt, px):
    """the generated mip chain (glz_host_mip_level, the product's host builder; tested against the blit rule elsewhere)"""
    tex = abi.Texture()
    tex.format, tex.width, tex.height, tex.mip_levels = fmt, px.shape[1], px.shape[0], 1
    keep = np.ascontiguousarray(px)
    tex.pixels = keep.ctypes.data
    levels = []
    for level in range(32):
        w, h = C.c_uint32(), C.c_uint32()
        n = abi.check(abi.lib().glz_host_mip_level(C.byref(tex), level, None, 0, C.byref(w), C.byref(h)))
        if n == 0:
            break
        out = np.zeros(n, np.uint8)
        abi.check(abi.lib().glz_host_mip_level(C.byref(tex), level, out.ctypes.data, n, C.byref(w), C.byref(h)))
        levels.append(texref.decode(fmt, out.reshape(h.value, w.value) if fmt == abi.TEX_GRAY else out.reshape(h.value, w.value, 4)))
    return levels


def footprints(w, h, seed):
    """(uv (n, 2), footprint (n, 4)): level 0, fractional levels, above the chain, NaN and -inf levels; taps 1..16; small and huge
    du / dv"""
    rng = np.random.default_rng(seed)
    base0 = -0.5 * np.log2(w * h)                      # lod_base of level 0 exactly
    bases = np.array([-1e30, base0 - 3, base0, base0 + 0.37, base0 + 1.5, base0 + 2.71, base0 + 40, np.nan, -np.inf, np.inf], np.float32)
    rows = []
    for b in bases:
        for taps in (1, 2, 3, 5, 8, 16):
            for du, dv in ((0.0, 0.0), (0.3, -0.1), (-2.5, 7.0), (1e6, 3e-3), (-5e8, 2e9), (1e20, -1e20)):
                n = 24
                uv = rng.uniform(-4, 4, (n, 2))
                rows.append(np.concatenate([uv, np.tile([b, du, dv, taps], (n, 1))], 1))
    a = np.concatenate(rows).astype(np.float32)
    return a[:, :2].copy(), a[:, 2:].copy()


@pytest.mark.parametrize("k", LOD_TEXTURES)
def test_oracle_lod_matches_float64_reference(oracle_sampler, k):
    desc, sc = oracle_sampler
    w, h, fmt = SIZES[k]
    uv, fp = footprints(w, h, k)
    got = sc.sample_texture(k + 1, uv, fp)
    want, bound = texref.lod(host_levels(fmt, desc.textures[k + 1][1]), uv[:, 0], uv[:, 1], fp[:, 0], fp[:, 1], fp[:, 2], fp[:, 3].astype(np.int64))
    nan_want = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan_want), "NaN results differ from the reference"
    ok = ~nan_want
    err = np.abs(got.astype(np.float64) - want)
    bad = ok & (err > bound)
    assert not bad.any(), "%d lod fetches off the float64 reference, e.g. uv %s footprint %s got %s want %s bound %s" % (
        bad.any(1).sum(), uv[bad.any(1)][0], fp[bad.any(1)][0], got[bad.any(1)][0], want[bad.any(1)][0], bound[bad.any(1)][0])


# ---- the device ---------------------------------------------------------------------------------------------------------------
def assert_same(g, c, what):
    assert np.array_equal(np.isnan(g), np.isnan(c)), what + ": NaN results differ"
    ok = ~np.isnan(c)
    diff = g[ok].view(np.uint32) != c[ok].view(np.uint32)
    assert not diff.any(), "%s: %d values differ from the oracle" % (what, diff.sum())


@pytest.mark.gpu
def test_device_sampler_equals_oracle(instance):
    desc = sampler_desc()
    gpu, sc = glaze_amd.RayTraceScene.from_desc(instance, desc), OracleScene(desc)
    for k, (w, h, fmt) in enumerate(SIZES):
        for huge in (False, True):
            u, v = coordinates(w, h, k, huge_only=huge)
            uv = np.stack([u, v], -1)
            g = gpu.debug_sample_texture(k + 1, uv)
            assert_same(g, sc.sample_texture(k + 1, uv), "level 0, %dx%d fmt %d%s" % (w, h, fmt, " huge" if huge else ""))
            check_against_reference(g, desc.textures[k + 1][1], fmt, u, v, "device %dx%d fmt %d" % (w, h, fmt))
    for k in LOD_TEXTURES:
        uv, fp = footprints(*SIZES[k][:2], k)
        assert_same(gpu.debug_sample_texture(k + 1, uv, fp), sc.sample_texture(k + 1, uv, fp), "lod, texture %d" % (k + 1))


@pytest.mark.gpu
def test_device_srgb_row_is_the_eotf(instance):
    gpu = glaze_amd.RayTraceScene.from_desc(instance, sampler_desc())
    u = (np.arange(256, dtype=np.float32) + np.float32(0.5)) / np.float32(256)
    got = gpu.debug_sample_texture(SRGB_ROW, np.stack([u, np.full(256, 0.5, np.float32)], -1))
    code = np.arange(256)
    assert np.array_equal(got[:, 0], texref.eotf(code / 255.0).astype(np.float32))
    assert np.array_equal(got[:, 1], texref.eotf(code[::-1] / 255.0).astype(np.float32))
    assert np.array_equal(got[:, 3], (code[::-1] / 255.0).astype(np.float32))


@pytest.mark.gpu
def test_device_sampler_large_texture_behind_others(instance):
    """A 4096 x 4096 RGBA texture after smaller ones: texel addresses pass 2^26 bytes (its far corner, every wrap across it)"""
    rng = np.random.default_rng(5)
    big = rng.integers(0, 256, (4096, 4096, 4), dtype=np.uint8)
    desc = textured_desc([(abi.TEX_GRAY, texture_pixels(17, 9, abi.TEX_GRAY, 1)), (abi.TEX_RGBA_NORM, texture_pixels(130, 66, abi.TEX_RGBA_NORM, 2)),
                          (abi.TEX_RGBA_SRGB, big), (abi.TEX_GRAY, texture_pixels(9, 5, abi.TEX_GRAY, 3))])
    gpu, sc = glaze_amd.RayTraceScene.from_desc(instance, desc), OracleScene(desc)
    edge = (np.array([0, 1, 2, 7, 8, 4087, 4088, 4094, 4095], np.float64) + 0.5) / 4096
    u, v = np.meshgrid(np.concatenate([edge, edge + 0.3 / 4096, [1.0, -1e-7]]), np.concatenate([edge, edge - 0.4 / 4096, [0.9999999]]))
    u, v = np.concatenate([u.ravel(), rng.uniform(-2, 2, 20000)]).astype(np.float32), np.concatenate([v.ravel(), rng.uniform(-2, 2, 20000)]).astype(np.float32)
    cu, cv = coordinates(4096, 4096, 9, huge_only=True)
    u, v = np.concatenate([u, cu]), np.concatenate([v, cv])
    uv = np.stack([u, v], -1)
    g = gpu.debug_sample_texture(3, uv)
    assert_same(g, sc.sample_texture(3, uv), "4096 x 4096")
    check_against_reference(g, big, abi.TEX_RGBA_SRGB, u, v, "device 4096 x 4096")


# ---- one render at huge texture coordinates -----------------------------------------------------------------------------------
def far_uv_plane(texture):
    """A square facing the camera whose vt are about 1e7 (u w about 2.6e9 on a 256-texel texture), Lambert with `texture` as diffuse map"""
    p = [(-1.0, -1.0, 3.0), (1.0, -1.0, 3.0), (1.0, 1.0, 3.0), (-1.0, 1.0, 3.0)]
    t = [(1.0e7, 1.0e7), (1.0e7 + 64.0, 1.0e7), (1.0e7 + 64.0, 1.0e7 + 64.0), (1.0e7, 1.0e7 + 64.0)]
    vertices = np.zeros(4, VERTEX_DTYPE)
    for i in range(4):
        vertices[i] = (p[i], (0.0, 0.0, -1.0), t[i])
    materials = [make_material("default"), make_material("plane", mtype=abi.MAT_LAMBERT, diffuse=1)]
    texs = [(abi.TEX_RGBA_SRGB, np.full((1, 1, 4), 255, np.uint8), "default"), (abi.TEX_RGBA_SRGB, texture, "plane")]
    lights = [make_light(abi.LIGHT_SUN, "sun", direction=(0.3, -0.2, 1.0), intensity=1.0)]
    camera = make_camera(position=(0, 0, 0), target=(0, 0, 1), up=(0, 1, 0), fovx=np.float32(np.radians(50.0)), near=1e-3, far=100.0)
    return SceneDesc(vertices, np.array([0, 2, 1, 0, 3, 2], np.uint32), np.array([(0, 1, 0, 6)], MESH_DTYPE), None,
                     np.array([(0, 0)], INSTANCE_DTYPE), materials, lights, texs, camera, make_meta(centre=(0, 0, 3), radius=4.0))


@pytest.mark.gpu
def test_render_at_huge_texture_coordinates(instance):
    from test_gpu_render import assert_parity, render_both
    rng = np.random.default_rng(11)
    bw = np.where(rng.integers(0, 2, (256, 256)) == 1, 255, 0).astype(np.uint8)
    checker = np.stack([bw, bw, bw, np.full_like(bw, 255)], -1)
    r, o, _ = render_both(instance, far_uv_plane(checker), 64, 64, 8, depth=1, integrator=glaze_amd.Integrator.DIRECT)
    assert_parity(r, o, "vt ~ 1e7")
    rw, ow, _ = render_both(instance, far_uv_plane(np.full((256, 256, 4), 255, np.uint8)), 64, 64, 8, depth=1, integrator=glaze_amd.Integrator.DIRECT)
    a, b = r.read_hdr()[..., :3], rw.read_hdr()[..., :3]
    assert np.isfinite(a).all() and (b > 0).any()
    assert (a <= b * (1 + 1e-6) + 1e-30).all(), "a black / white texture lit more than a white one"
