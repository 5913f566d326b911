"""Which hits the "det is rounding noise" rule may drop, pinned from OUTSIDE the oracle.

oracle.cpp ray_tri = device/intersect.h triangle_finish leave a candidate out when |U + V + W| is not above 2^-19 of
(|first product of U| + |of V| + |of W|): the ray lies in the triangle's plane as far as single precision can tell.  The reference's
hits come from the driver's intersector, which has no such rule, so the rule must only ever take what no intersector in floats could
decide anyway.  Here a float64 statement of ray / triangle intersection (plane equation + barycentrics, nothing shared with the
oracle) says which rays hit which triangle; the oracle (CPU) and the HIP tracer (GPU) must agree with it on
  * grazing rays: every ray that meets its triangle well inside (barycentrics >= 0.05) at an angle to the plane whose sine is >= 1e-5
    is a hit of that triangle, at the float64 distance within the conditioning of a grazing ray (relative error <= 4e-7 / sine) -- in
    this sample every such ray down to a sine of 1e-6 is reported, 84 % of those between 1e-7 and 1e-6, 12 % below 1e-7: the rule
    bites where the ROUNDED ray is no longer distinguishable from one in the plane;
  * slivers: a ray straight through the middle of a triangle whose sides are up to 1 : 100 000 is a hit (measured: all of them up to an
    aspect of 5e5 : 1 of the projected triangle, 99 % up to 5e6 : 1);
  * and in the zone the rule may take -- sines below 1e-7, aspects above 5e6 -- whatever is reported is reported by everybody alike
    (oracle hierarchy = oracle walk over all triangles = HIP), and a reported hit is never a triangle the ray misses by more than the
    triangle's own size.
"""
import numpy as np
import pytest

from glaze_amd.scene_desc import INSTANCE_DTYPE, MESH_DTYPE, VERTEX_DTYPE, SceneDesc
from oracle.pyoracle import OracleScene

N = 4000


def _scene(pos, tri):
    v = np.zeros(len(pos), VERTEX_DTYPE)
    v["vv"], v["vn"], v["vt"] = pos, (0, 1, 0), 0.5
    tri = np.asarray(tri, np.uint32).reshape(-1)
    return SceneDesc(v, tri, np.array([(0, 0, 0, tri.size)], MESH_DTYPE), None, np.array([(0, 0)], INSTANCE_DTYPE))


def _case(kind, seed):
    """N triangles, one per cell of a coarse lattice (so a ray aimed at one cannot meet another on its way), and one ray for each.
    Returns desc, origins, dirs (float32), and per ray: the triangle aimed at, the float64 distance, the sine of the angle between ray and
    plane, the triangle's aspect as the ray sees it."""
    rng = np.random.default_rng(seed)
    cell = np.stack(np.unravel_index(np.arange(N), (16, 16, 16)), 1).astype(np.float64) * 8.0 - 60.0
    q = rng.normal(size=(N, 3)); q /= np.linalg.norm(q, axis=1, keepdims=True)          # plane normal
    e1 = np.cross(q, rng.normal(size=(N, 3))); e1 /= np.linalg.norm(e1, axis=1, keepdims=True)
    e2 = np.cross(q, e1)
    size = rng.uniform(0.2, 1.5, N)
    if kind == "grazing":
        thin = np.ones(N)
        sine = 10.0 ** rng.uniform(-8.5, -0.3, N)
    else:
        thin = 10.0 ** -rng.uniform(0.0, 8.0, N)                                        # the triangle's height over its base
        sine = np.ones(N)
    a = cell + rng.uniform(-0.5, 0.5, (N, 3))
    b = a + e1 * size[:, None]
    c = a + e1 * (0.4 * size)[:, None] + e2 * (size * thin)[:, None]
    pos = np.stack([a, b, c], 1).astype(np.float32)                                      # what everybody sees: the ROUNDED vertices
    A, B, C = (pos[:, k].astype(np.float64) for k in range(3))
    nrm = np.cross(B - A, C - A)
    area2 = np.linalg.norm(nrm, axis=1)
    nrm /= np.maximum(area2, 1e-300)[:, None]
    w = rng.dirichlet((4.0, 4.0, 4.0), N) * 0.85 + 0.05                                  # barycentrics >= 0.05
    p = A * w[:, :1] + B * w[:, 1:2] + C * w[:, 2:]
    along = (B - A) / np.linalg.norm(B - A, axis=1, keepdims=True)
    along = along * np.cos(rng.uniform(0, 2 * np.pi, N))[:, None] + np.cross(nrm, along) * np.sin(rng.uniform(0, 2 * np.pi, N))[:, None]
    along /= np.linalg.norm(along, axis=1, keepdims=True)
    cosine = np.sqrt(np.maximum(0.0, 1.0 - sine * sine))
    d = -(along * cosine[:, None] + nrm * sine[:, None])                                 # towards the plane from above
    dist = rng.uniform(0.5, 2.5, N)
    o32 = (p - d * dist[:, None]).astype(np.float32)
    d32 = d.astype(np.float32)
    # float64 truth for the ROUNDED ray against the ROUNDED triangle it aims at
    o, dd = o32.astype(np.float64), d32.astype(np.float64)
    denom = np.einsum("ij,ij->i", nrm, dd)
    denom = np.where(denom == 0.0, 1e-300, denom)
    t = np.einsum("ij,ij->i", nrm, A - o) / denom
    hp = o + dd * t[:, None]
    def bary(P, Q, R):
        return np.einsum("ij,ij->i", np.cross(Q - P, R - P), nrm) / np.maximum(area2, 1e-300)
    w0, w1, w2 = bary(hp, B, C), bary(A, hp, C), bary(A, B, hp)
    inside = (np.minimum(np.minimum(w0, w1), w2) > 0.02) & (t > 1e-3)
    with np.errstate(all="ignore"):      # (a sliver that rounds to a segment has no normal: its ray is excluded by `inside` below)
        true_sine = np.abs(denom) / np.linalg.norm(dd, axis=1)
    # the projected triangle's aspect: longest side over the height the ray sees
    longest = np.maximum(np.maximum(np.linalg.norm(B - A, axis=1), np.linalg.norm(C - B, axis=1)), np.linalg.norm(A - C, axis=1))
    with np.errstate(all="ignore"):
        aspect = longest * longest / np.maximum(area2 * true_sine, 1e-300)
    tri = np.arange(3 * N, dtype=np.uint32)
    return _scene(pos.reshape(-1, 3), tri), o32, d32, np.arange(N), t, true_sine, aspect, inside, (A, B, C, nrm)


def _check(trace_closest, who):
    reports = []
    for kind, seed in (("grazing", 11), ("sliver", 12)):
        desc, o, d, aim, t64, sine, aspect, inside, (A, B, C, nrm) = _case(kind, seed)
        t, tri = trace_closest(desc, o, d)
        hit = np.isfinite(t)
        reports.append((t.copy(), tri.copy()))
        if kind == "grazing":
            must = inside & (sine >= 1e-5)
            assert must.sum() > 0.5 * N
            assert hit[must].all() and (tri[must] == aim[must]).all(), who + ": a grazing ray well above the rule's threshold lost its hit"
            assert (np.abs(t[must] - t64[must]) <= (4e-7 / sine[must] + 4e-6) * np.maximum(np.abs(t64[must]), 1.0) * 8.0).all(), who + ": grazing distance"
            assert (sine < 1e-6).sum() > 300   # the rule's own territory is sampled (of the rays there that still meet their triangle in float64, 84 % are reported at sines of 1e-7 ... 1e-6 and 12 % below); nothing is required of them here but consistency
        else:
            must = inside & (aspect <= 1e5)
            assert must.sum() > 0.4 * N
            assert hit[must].all() and (tri[must] == aim[must]).all(), who + ": a ray through a sliver of aspect <= 1e5 lost its hit"
            # the sheared coordinates across a sliver are differences of O(1) numbers: the barycentrics carry ~1e-7 x aspect, and with the
            # ROUNDED sliver tilted against the ray by up to its own height over the coordinates' ulp the distance inherits it
            assert (np.abs(t[must] - t64[must]) <= 5e-6 + 4e-9 * aspect[must]).all(), who + ": sliver distance"
        # a reported hit is never on a triangle the ray misses by more than that triangle's size, nor on another cell's triangle
        near = hit & (t < 4.0)             # (a ray that misses its own triangle may fly on into another cell, 8 units away: a true hit)
        assert (tri[near] == aim[near]).all(), who + ": a ray hit a triangle it was not aimed at"
        far = near & ~inside
        if far.any():
            hp = o[far].astype(np.float64) + d[far].astype(np.float64) * t[far, None].astype(np.float64)
            size = np.maximum(np.linalg.norm(B[far] - A[far], axis=1), np.linalg.norm(C[far] - A[far], axis=1))
            assert (np.linalg.norm(hp - A[far], axis=1) <= 3.0 * size).all(), who + ": a phantom hit far outside its triangle"
    return reports


def test_oracle_drops_only_what_single_precision_cannot_decide():
    scenes = {}

    def via(brute):
        def f(desc, o, d):
            key = id(desc)
            if key not in scenes:
                scenes[key] = OracleScene(desc)
            r = scenes[key].trace_closest(o, d, brute=brute)
            return r[0], r[1]
        return f
    a = _check(via(False), "oracle hierarchy")
    scenes.clear()
    b = _check(via(True), "oracle walk over all triangles")
    for (ta, ia), (tb, ib) in zip(a, b):
        assert np.array_equal(ta.view(np.uint32), tb.view(np.uint32)) and np.array_equal(ia[np.isfinite(ta)], ib[np.isfinite(tb)])


@pytest.mark.gpu
def test_hip_drops_exactly_what_the_oracle_drops(instance):
    import glaze_amd
    keep = []

    def hip(desc, o, d):
        sc = glaze_amd.RayTraceScene.from_desc(instance, desc)
        keep.append(sc)
        r = sc.debug_trace_closest(o, d)
        return r[0], r[1]
    a = _check(hip, "hip")
    scenes = []

    def orc(desc, o, d):
        s = OracleScene(desc)
        scenes.append(s)
        r = s.trace_closest(o, d, brute=True)
        return r[0], r[1]
    b = _check(orc, "oracle")
    for (ta, ia), (tb, ib) in zip(a, b):
        assert np.array_equal(ta.view(np.uint32), tb.view(np.uint32)) and np.array_equal(ia[np.isfinite(ta)], ib[np.isfinite(tb)])
