"""The multi-bounce loop of the path integrator against a closed form in a CLOSED room (the open scenes, one non-specular vertex each, are
in test_analytic_render.py and test_analytic_render2.py): the inside of a Lambertian sphere of radius R lit by one point light.

Why it has a closed form.  Between any two points of a sphere's inside the form factor is the constant 1 / (4 pi R^2): a cosine-sampled
direction from any surface point lands uniformly by area.  So the expected direct lighting at the end of a cosine-sampled bounce is the area
average of the irradiance, and for an omni light of intensity I anywhere inside that is I / R^2 (its flux 4 pi I lands on 4 pi R^2).  A
cosine-sampled Lambert bounce multiplies the importance by value x |cos| / pdf = (albedo / pi) x cos / (cos / pi) = the albedo spectrum rho.
What is left is the bookkeeping of path_trace.rgen:135-239, restated here launch by launch for one pixel (D = pt_steps):

    state s = 0 .. D: the value of hit[3] when the launch starts; every ray hits, the room is closed
    a launch in state s adds      imp_s x value x emission x E_s          imp_0 = 1, E_0 = E_direct(first hit), E_s = I / R^2 for s >= 1
    if s > D // 2:                kill = max(0.05, 1 - luminance(imp_s)); the path ends here with probability kill, else imp_s /= 1 - kill
    then                          imp_{s+1} = imp_s x rho, and the next launch is in state s + 1 if s < D, else in state 0 (the wrap: a path
                                  has D + 1 vertices, and the roulette of state D decides nothing)
    EVERY launch adds 1 to the pixel's sample count

    reach_0 = 1, reach_{s+1} = reach_s x (1 - kill_s)
    converged pixel = sum_s reach_s x (what state s adds) / sum_s reach_s           (renewal-reward: a path of k launches is counted k times)

The same chain propagated over exactly N launches from state 0 (occupancy of every state at every launch, in closed form, no sampling) is
the expectation of the image after N launches; it tends to the converged pixel like 1 / N (asserted), and it is what a render of N launches
is compared with, so that the start-up transient is accounted for and not left to eat into the interval.

What is taken from the oracle's own routines, as in the other analytic files, is only spectral: bsdf_value for `value`, light_sample at
unit distance for the emission, orc_dev_rgb for spectrum -> RGB, orc_dev_luminance for the roulette's luminance (test_oracle_math.py checks
those against the formulas).  Geometry, cosines, 1 / d^2, rho = pi x value, the roulette rule, the wrap and the launch accounting are here.

The mesh bracket.  The mesh is an icosphere with FLAT normals (unshared vertices that carry their facet's inward normal: with smooth normals
a direction sampled about the shading normal can point below the facet and leave the mesh -- the reference's behaviour, but without a closed
form; the smooth sphere gets a parity test and a one-sided bound only).  A facet lies inside the sphere, so every E above is bracketed, not
exact.  Light at the centre: a point of a facet at plane distance h from the centre, at distance d in [h, R], receives I h / d^3, between
I h_min / R^3 and I / h_min^2.  Light off the centre: I cos_facet / d^2 is compared with the true sphere's value at the radial projection of
the same point (what the same camera ray sees), at every facet's vertices, edge midpoints, centroid and the feet of the perpendiculars from the
centre and from the light, and the smallest and largest ratio bracket every term.  [lo, hi] multiplies the numerator only: the denominator
(the occupancy of the states) does not depend on geometry.

The acceptance interval is derived, not chosen:  lo (1 - 5 sigma) <= got <= hi (1 + 5 sigma)  for the image mean (all three channels) and for
the mean of every b x b block of pixels (green).  sigma is the relative standard error of that mean, measured on NEITHER renderer but on an
independent float64 simulation of the chain above with numpy's generator (seeded): 200 trials of b x b pixels x N launches, simulated launch by
launch; a block trial is evaluated as it stands, and because pixels are independent chains the variance of the mean over the P pixels of the
image is the sum of the pixels' variances over P^2, taken from the same 12 800 simulated chains (their counts of state-0 launches and their
indirect sums, and each pixel's own E_0).  With the light off the centre the indirect E_s are drawn at uniformly distributed points of the
true sphere (where cosine-weighted directions land) and the variance of E_0 inside a pixel is added per state-0 launch.  The factor 5: a suite
with a few dozen such comparisons raises a false alarm in fewer than one of 10^5 runs.

Discriminating power is a condition of every case, not a measurement: the same recursion gives what these misreadings would converge to --
    nocomp   the importance of a roulette survivor is not divided by 1 - kill
    ge       roulette from s >= D // 2 on
    short    a path of D vertices (wrap at hit[3] < D - 1)
    nofloor  kill = max(0, 1 - luminance): no 0.05 floor
    perpath  the textbook normalisation: the sum divided by the number of camera rays, not by the number of launches
-- and each case asserts that every mutant it CLAIMS lies outside its acceptance interval for the image mean by at least the interval's own
width.  The cases (subdivisions, launches, frames, bracket width hi / lo - 1, measured sigma of the image mean, claimed mutants); sigma as
measured by the simulation with seed 2024, CPU frame / GPU frame:

    case                   subd launches   bracket   sigma (24^2 / 128^2)   claimed (both frames)
    centre-albedo150-D1       4     1500    0.342%     0.0000% / 0.0000%   ge short perpath
    centre-albedo150-D2       4     1500    0.342%     0.0000% / 0.0000%   ge short perpath
    centre-albedo150-D5       4     1500    0.342%     0.0034% / 0.0006%   nocomp ge perpath
    centre-albedo150-D6       4     1500    0.342%     0.0075% / 0.0014%   nocomp ge perpath
    centre-albedo150-D7       4     1500    0.342%     0.0093% / 0.0017%   nocomp ge perpath
    centre-albedo150-D12      4     1500    0.342%     0.0149% / 0.0028%   nocomp ge perpath
    centre-albedo252-D1       5     1500    0.085%     0.0000% / 0.0000%   ge short perpath
    centre-albedo252-D2       5     1500    0.085%     0.0000% / 0.0000%   ge short perpath
    centre-albedo252-D5       5     1500    0.085%     0.0006% / 0.0001%   nocomp ge short nofloor perpath
    centre-albedo252-D6       5     1500    0.085%     0.0006% / 0.0001%   nocomp ge short nofloor perpath
    centre-albedo252-D7       5     1500    0.085%     0.0013% / 0.0002%   nocomp ge short nofloor perpath
    centre-albedo252-D12      5     1500    0.085%     0.0045% / 0.0008%   nocomp ge short nofloor perpath
    offcentre-albedo150-D6    5     1500    2.771%     0.0385% / 0.0072%   ge perpath
    offcentre-albedo252-D6    5     1500    2.771%     0.0601% / 0.0113%   perpath

Each mutant was also applied, one at a time, to a scratch copy of oracle/oracle.cpp when this file was written, and the oracle cases that
failed were the ones that claim it (and a few more through their blocks): nocomp -- all eight centre cases with D >= 5 and both off-centre
ones; ge and perpath -- all fourteen; short -- D = 1, 2 at both albedos, D >= 5 at albedo 252 (and D = 5, 6 at 150, off-centre 252);
nofloor -- D = 5, 6, 7, 12 at albedo 252.  The unmodified oracle and the HIP path in both launch modes sit at 1.0012 (4 subdivisions) and
1.0003 (5) times the true sphere's value: inside the bracket, above 1 because the facets catch the same flux on a smaller area.
"""
import functools

import numpy as np
import pytest

import glaze_amd
from glaze_amd import abi
from glaze_amd.scene_desc import INSTANCE_DTYPE, MESH_DTYPE, VERTEX_DTYPE, make_light, make_meta
from glaze_amd.scenes import cube_scene
from oracle import pyoracle
from oracle.pyoracle import OracleRenderer, OracleScene

ROOM_MAT = 2
R = 2.0
INTENSITY = 0.8
CENTRE, OFF_CENTRE = (0.0, 0.0, 0.0), (0.0, 0.0, R / 2)
LAUNCHES = 1500
CPU_FRAME, GPU_FRAME, BLOCK = 24, 128, 8
TRIALS, SIM_SEED = 200, 2024
MUTANTS = ("nocomp", "ge", "short", "nofloor", "perpath")

# (light, albedo, D) -> (subdivisions, mutants claimed: on the CPU frame and on the GPU frame alike)
CASES = {
    (CENTRE, 150, 1): (4, ("ge", "short", "perpath")),
    (CENTRE, 150, 2): (4, ("ge", "short", "perpath")),
    (CENTRE, 150, 5): (4, ("nocomp", "ge", "perpath")),
    (CENTRE, 150, 6): (4, ("nocomp", "ge", "perpath")),
    (CENTRE, 150, 7): (4, ("nocomp", "ge", "perpath")),
    (CENTRE, 150, 12): (4, ("nocomp", "ge", "perpath")),
    (CENTRE, 252, 1): (5, ("ge", "short", "perpath")),
    (CENTRE, 252, 2): (5, ("ge", "short", "perpath")),
    (CENTRE, 252, 5): (5, ("nocomp", "ge", "short", "nofloor", "perpath")),
    (CENTRE, 252, 6): (5, ("nocomp", "ge", "short", "nofloor", "perpath")),
    (CENTRE, 252, 7): (5, ("nocomp", "ge", "short", "nofloor", "perpath")),
    (CENTRE, 252, 12): (5, ("nocomp", "ge", "short", "nofloor", "perpath")),
    (OFF_CENTRE, 150, 6): (5, ("ge", "perpath")),
    (OFF_CENTRE, 252, 6): (5, ("perpath",)),
}


# ---------------------------------------------------------------------------------------------------------------------
# the room
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def icosphere(subdivisions):
    """float64 vertices on the sphere of radius R and triangles wound so that (b - a) x (c - a) points INWARD"""
    t = (1.0 + np.sqrt(5.0)) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    verts = [np.array(p, np.float64) / np.linalg.norm(p) for p in v]
    faces = f
    for _ in range(subdivisions):
        mid, nxt = {}, []

        def midpoint(i, j):
            key = (min(i, j), max(i, j))
            if key not in mid:
                m = verts[i] + verts[j]
                verts.append(m / np.linalg.norm(m))
                mid[key] = len(verts) - 1
            return mid[key]

        for a, b, c in faces:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            nxt += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        faces = nxt
    p = np.array(verts) * R
    tri = np.array(faces)
    a, b, c = p[tri[:, 0]], p[tri[:, 1]], p[tri[:, 2]]
    outward = (np.cross(b - a, c - a) * (a + b + c)).sum(-1) > 0
    tri[outward] = tri[outward][:, [0, 2, 1]]
    return p, tri


def facets(subdivisions):
    """corners (n, 3, 3), inward unit normals (n, 3) and plane distances from the centre (n) of the icosphere's facets, float64"""
    p, tri = icosphere(subdivisions)
    corners = p[tri]
    n = np.cross(corners[:, 1] - corners[:, 0], corners[:, 2] - corners[:, 0])
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    h = -(n * corners[:, 0]).sum(-1)
    assert (h > 0.75 * R).all() and (h < R).all()
    return corners, n, h


def sphere_room(subdivisions, light_pos, albedo, flat=True, parts=1):
    """cube_scene()'s camera (at the origin, looking down + z, 90 degrees), textures and materials around the icosphere; `parts` > 1 splits
    the facets into that many meshes, one identity instance each"""
    desc = cube_scene(material_type=abi.MAT_LAMBERT)
    m = desc.materials[ROOM_MAT]
    m.diffuse = 0                                                         # the 1 x 1 white texture: the colour is diffuse_mul
    m.diffuse_mul[:3] = (albedo, albedo, albedo)
    p, tri = icosphere(subdivisions)
    if flat:
        corners, n, _ = facets(subdivisions)
        vertices = np.zeros(3 * len(tri), VERTEX_DTYPE)
        vertices["vv"] = corners.reshape(-1, 3)
        vertices["vn"] = np.repeat(n, 3, axis=0)
        indices = np.arange(3 * len(tri), dtype=np.uint32)
    else:
        vertices = np.zeros(len(p), VERTEX_DTYPE)
        vertices["vv"] = p
        vertices["vn"] = -p / R
        indices = tri.astype(np.uint32).reshape(-1)
    vertices["vt"] = 0.5
    bounds = [len(tri) * k // parts for k in range(parts + 1)]
    desc.vertices = vertices
    desc.indices = indices
    desc.meshes = np.array([(k, ROOM_MAT, 3 * bounds[k], 3 * (bounds[k + 1] - bounds[k])) for k in range(parts)], MESH_DTYPE)
    desc.instances = np.array([(k, 0) for k in range(parts)], INSTANCE_DTYPE)
    desc.lights = [make_light(abi.LIGHT_OMNI, "in the room", position=tuple(light_pos), intensity=INTENSITY)]
    desc.meta = make_meta(centre=(0, 0, 0), radius=R, exposure=1.0)
    return desc


# ---------------------------------------------------------------------------------------------------------------------
# the reference: float64
# ---------------------------------------------------------------------------------------------------------------------
def spectrum_rgb(sp):
    out = np.zeros(3, np.float32)
    sp = np.ascontiguousarray(sp, np.float32)
    pyoracle.lib().orc_dev_rgb(sp.ctypes.data, out.ctypes.data)
    return out.astype(np.float64)


def luminance(sp):
    sp = np.ascontiguousarray(sp, np.float32)
    return float(pyoracle.lib().orc_dev_luminance(sp.ctypes.data))


@functools.lru_cache(maxsize=None)
def spectra(albedo, light_pos):
    """(Lambert value of the wall, emission of the light at unit distance) as spectra: the oracle's spectral routines"""
    o = OracleScene(sphere_room(0, light_pos, albedo))
    up = np.array([[0.0, 0.0, 1.0]], np.float32)
    value, pdf = o.bsdf_value(ROOM_MAT, up, up)
    assert pdf[0] > 0
    at = np.asarray(light_pos, np.float32) + np.array([1.0, 0.0, 0.0], np.float32)
    _, dist, lpdf, em = o.light_sample(0, at[None, :], np.zeros((1, 3), np.float32), scene_radius=R)
    assert dist[0] == 1.0 and lpdf[0] == 1.0
    return value[0].astype(np.float64), em[0].astype(np.float64)


@functools.lru_cache(maxsize=None)
class Chain:
    """The state recursion for one albedo, light and depth D, optionally misread (`mutant`).  a[s]: RGB that a launch in state s adds per unit
    of E_s; kill[s]: the probability that the path ends in state s; `last`: the state after which the counter wraps."""

    def __init__(self, albedo, light_pos, D, mutant=None):
        value, em = spectra(albedo, light_pos)
        rho = np.pi * value
        self.D, self.mutant = D, mutant
        self.last = D - 1 if mutant == "short" else D
        first = D // 2 if mutant == "ge" else D // 2 + 1                   # the first state that plays roulette
        imp = np.ones(16)
        self.a, self.kill = [], []
        for s in range(self.last + 1):
            self.a.append(spectrum_rgb(imp * value * em))
            k = 0.0
            if s >= first:
                k = max(0.0 if mutant == "nofloor" else 0.05, 1.0 - luminance(imp))
                if mutant != "nocomp":
                    imp = imp / (1.0 - k)
            self.kill.append(k)
            imp = imp * rho
        self.a, self.kill = np.array(self.a), np.array(self.kill)
        self.reach = np.concatenate([[1.0], np.cumprod(1.0 - self.kill[:-1])])

    def converged(self, e0, e_ind):
        """the converged pixel, RGB in the last axis, for E_0 = e0 (any shape) and E_s = e_ind"""
        num = np.asarray(e0)[..., None] * self.a[0] + e_ind * (self.reach[1:, None] * self.a[1:]).sum(0)
        return num if self.mutant == "perpath" else num / self.reach.sum()

    @functools.lru_cache(maxsize=None)
    def occupancy(self, launches):
        """expected number of launches, out of the first `launches` from a fresh pixel, that start in each state"""
        p = np.zeros(self.last + 1)
        p[0] = 1.0
        total = np.zeros_like(p)
        for _ in range(launches):
            total += p
            q = np.zeros_like(p)
            q[1:] = p[:-1] * (1.0 - self.kill[:-1])
            q[0] = 1.0 - q[1:].sum()
            p = q
        return total

    def expected(self, e0, e_ind, launches):
        """expectation of the pixel after exactly `launches` launches"""
        occ = self.occupancy(launches)
        num = np.asarray(e0)[..., None] * (occ[0] * self.a[0]) + e_ind * (occ[1:, None] * self.a[1:]).sum(0)
        return num / (occ[0] if self.mutant == "perpath" else launches)


def pixel_grid(n, sub):
    c = (np.arange(n * sub) + 0.5) / (n * sub) * 2.0 - 1.0                # tan(45 deg) = 1: image plane coordinates at distance 1
    return np.meshgrid(c, c, indexing="xy")


def sphere_irradiance(points, light_pos):
    """cos / d^2 at points of the TRUE sphere, normal - p / R (the intensity I is part of the emission at unit distance)"""
    w = np.asarray(light_pos) - points
    d2 = (w * w).sum(-1)
    return (w * (-points / R)).sum(-1) / d2 ** 1.5


@functools.lru_cache(maxsize=None)
def direct_term(n, light_pos, sub=8):
    """(mean, variance) inside each pixel of E_direct at the first hit on the true sphere: the camera is at the centre, so the hit is R x
    the ray's direction.  The light is on the camera's axis: the form does not depend on how the image axes are oriented."""
    u, v = pixel_grid(n, sub)
    d = np.stack([u, v, np.ones_like(u)], -1)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    e = sphere_irradiance(R * d, light_pos).reshape(n, sub, n, sub)
    return e.mean(axis=(1, 3)), e.var(axis=(1, 3))


@functools.lru_cache(maxsize=None)
def mesh_bracket(subdivisions, light_pos):
    """(lo, hi): every irradiance on the mesh lies between lo x and hi x the true sphere's"""
    corners, n, h = facets(subdivisions)
    if tuple(light_pos) == CENTRE:
        return h.min() / R, (R / h.min()) ** 2                             # I h / d^3, d in [h, R], against I / R^2
    light = np.asarray(light_pos)
    a, b, c = corners[:, 0], corners[:, 1], corners[:, 2]
    foot_centre = -n * h[:, None]
    foot_light = light - n * ((light - a) * n).sum(-1, keepdims=True)
    inside = []
    for q in (foot_centre, foot_light):                                    # a foot outside its facet is replaced by the centroid
        ok = np.ones(len(q), bool)
        for p0, p1 in ((a, b), (b, c), (c, a)):
            ok &= (np.cross(p1 - p0, q - p0) * n).sum(-1) >= 0
        inside.append(np.where(ok[:, None], q, (a + b + c) / 3))
    pts = np.stack([a, b, c, (a + b) / 2, (b + c) / 2, (c + a) / 2, (a + b + c) / 3] + inside, 1)        # (facets, 9, 3)
    w = light - pts
    d2 = (w * w).sum(-1)
    on_mesh = (w * n[:, None, :]).sum(-1) / d2 ** 1.5
    ratio = on_mesh / sphere_irradiance(pts * (R / np.linalg.norm(pts, axis=-1, keepdims=True)), light)
    assert (on_mesh > 0).all()
    return ratio.min(), ratio.max()


@functools.lru_cache(maxsize=None)
def simulate(albedo, light_pos, D, launches):
    """TRIALS x BLOCK^2 independent pixels simulated launch by launch with numpy's generator: per chain the number of launches in state 0
    and the RGB sum of what the launches in states >= 1 added (with E_s = 1 / R^2, or drawn)"""
    ch = Chain(albedo, light_pos, D)
    rng = np.random.default_rng(SIM_SEED)
    k = TRIALS * BLOCK * BLOCK
    s = np.zeros(k, np.int64)
    n0 = np.zeros(k)
    ind = np.zeros((k, 3))
    a_ind = ch.a.copy()
    a_ind[0] = 0.0
    for _ in range(launches):
        n0 += s == 0
        if tuple(light_pos) == CENTRE:
            ind += a_ind[s]
        else:                                                             # cosine-weighted directions land uniformly on the true sphere
            z = rng.uniform(-1.0, 1.0, k)
            phi = rng.uniform(0.0, 2.0 * np.pi, k)
            p = R * np.stack([np.sqrt(1.0 - z * z) * np.cos(phi), np.sqrt(1.0 - z * z) * np.sin(phi), z], -1)
            ind += a_ind[s] * (sphere_irradiance(p, light_pos) * R ** 2)[:, None]
        ends = (s == ch.last) | (rng.random(k) < ch.kill[s])
        s = np.where(ends, 0, s + 1)
    return n0, ind / R ** 2


class Reference:
    """Everything a case compares a render of `frame` x `frame` pixels with"""

    def __init__(self, light_pos, albedo, D, frame, launches=LAUNCHES):
        self.key, self.frame, self.launches = (tuple(light_pos), albedo, D), frame, launches
        self.subdivisions = CASES[self.key][0]
        self.chain = Chain(albedo, light_pos, D)
        self.e0, self.e0_var = direct_term(frame, tuple(light_pos))
        self.e_ind = 1.0 / R ** 2
        self.lo, self.hi = mesh_bracket(self.subdivisions, tuple(light_pos))
        assert self.lo <= 1.0 <= self.hi
        self.want = self.chain.expected(self.e0, self.e_ind, launches)     # (frame, frame, 3)
        limit = self.chain.converged(self.e0, self.e_ind)
        assert launches >= 50 * (D + 1) and np.abs(self.want / limit - 1.0).max() < 2.0 * (D + 1) / launches
        # sigma of the image mean per channel and of every block's mean (green), from the simulated chains
        n0, ind = simulate(albedo, tuple(light_pos), D, launches)
        a0 = self.chain.a[0]
        var_n0, mean_n0 = n0.var(ddof=1), n0.mean()
        var_pixels = np.zeros(3)
        for c in range(3):
            cov = np.cov(n0, ind[:, c])
            var_pixels[c] = (a0[c] ** 2 * (self.e0 ** 2 * var_n0 + mean_n0 * self.e0_var) + 2.0 * a0[c] * self.e0 * cov[0, 1] + cov[1, 1]).sum()
        self.sigma_image = np.sqrt(var_pixels) / frame ** 2 / launches / self.want.mean(axis=(0, 1))
        b, nb = BLOCK, frame // BLOCK
        blocks = lambda x: x.reshape(nb, b, nb, b).transpose(0, 2, 1, 3).reshape(nb * nb, b * b)
        trials = (np.einsum("tp,bp->bt", n0.reshape(TRIALS, b * b), blocks(self.e0)) * a0[1] + ind[:, 1].reshape(TRIALS, b * b).sum(-1)[None, :]) / (b * b * launches)
        jitter = a0[1] ** 2 * mean_n0 * blocks(self.e0_var).sum(-1) / (b * b * launches) ** 2
        self.want_blocks = self.want[..., 1].reshape(nb, b, nb, b).mean(axis=(1, 3))
        self.sigma_blocks = (np.sqrt(trials.var(axis=1, ddof=1) + jitter) / trials.mean(axis=1)).reshape(nb, nb)
        assert np.abs(trials.mean(axis=1).reshape(nb, nb) / self.want_blocks - 1.0).max() < 5.0 * self.sigma_blocks.max() / np.sqrt(TRIALS) + 1e-12

    def interval(self):
        """acceptance interval of the image mean, per channel"""
        mean = self.want.mean(axis=(0, 1))
        return self.lo * mean * (1.0 - 5.0 * self.sigma_image), self.hi * mean * (1.0 + 5.0 * self.sigma_image)

    def mutant_mean(self, mutant):
        light, albedo, D = self.key
        return Chain(albedo, light, D, mutant).expected(self.e0, self.e_ind, self.launches).mean(axis=(0, 1))

    def margin(self, mutant):
        """how far outside the interval of the image mean (green) the mutant lies, in widths of that interval"""
        lo, hi = self.interval()
        m = self.mutant_mean(mutant)[1]
        return max(lo[1] - m, m - hi[1]) / (hi[1] - lo[1])

    def check_power(self, claimed):
        for mutant in claimed:
            assert self.margin(mutant) >= 1.0, "%s is not told apart: %.2f widths outside" % (mutant, self.margin(mutant))

    def check(self, img):
        assert (img[..., 3] == self.launches).all()                       # every launch counts, whatever it added
        got = img[..., :3].astype(np.float64) / img[..., 3:4]
        assert np.isfinite(got).all()
        lo, hi = self.interval()
        mean = got.mean(axis=(0, 1))
        print("image mean / expected", mean / self.want.mean(axis=(0, 1)), "accepted", lo / self.want.mean(axis=(0, 1)), hi / self.want.mean(axis=(0, 1)))
        assert (lo <= mean).all() and (mean <= hi).all(), (mean, lo, hi)
        b, nb = BLOCK, self.frame // BLOCK
        gm = got[..., 1].reshape(nb, b, nb, b).mean(axis=(1, 3))
        rel = gm / self.want_blocks
        print("block means / expected: min %.5f max %.5f, sigma %.5f .. %.5f" % (rel.min(), rel.max(), self.sigma_blocks.min(), self.sigma_blocks.max()))
        assert (self.lo * (1.0 - 5.0 * self.sigma_blocks) <= rel).all() and (rel <= self.hi * (1.0 + 5.0 * self.sigma_blocks)).all(), (rel.min(), rel.max())


@functools.lru_cache(maxsize=None)
def reference(light_pos, albedo, D, frame):
    return Reference(light_pos, albedo, D, frame)


def case_id(key):
    return "%s-albedo%d-D%d" % ("centre" if key[0] == CENTRE else "offcentre", key[1], key[2])


ALL = pytest.mark.parametrize("key", list(CASES), ids=case_id)


# ---------------------------------------------------------------------------------------------------------------------
# the reference against itself
# ---------------------------------------------------------------------------------------------------------------------
def test_every_mutant_is_claimed_and_every_claim_holds():
    claimed = set()
    for key, (_, claims) in CASES.items():
        assert claims, "a case that tells nothing apart is removed"
        reference(*key, CPU_FRAME).check_power(claims)
        reference(*key, GPU_FRAME).check_power(claims)
        claimed |= set(claims)
    assert claimed == set(MUTANTS)


def test_the_mesh_is_closed_and_faces_inward_and_the_bracket_holds_at_random_points():
    for subdivisions in (4, 5):
        p, tri = icosphere(subdivisions)
        assert len(tri) == 20 * 4 ** subdivisions and np.allclose(np.linalg.norm(p, axis=1), R, rtol=0, atol=1e-12)
        edges = np.concatenate([tri[:, [0, 1]], tri[:, [1, 2]], tri[:, [2, 0]]])
        directed = set(map(tuple, edges))
        assert len(directed) == len(edges) and all((b, a) in directed for a, b in directed)     # every edge once in each direction
        corners, n, h = facets(subdivisions)
        rng = np.random.default_rng(1)
        w = rng.dirichlet((1.0, 1.0, 1.0), len(corners))
        pts = (corners * w[:, :, None]).sum(1)
        for light in (CENTRE, OFF_CENTRE):
            lo, hi = mesh_bracket(subdivisions, light)
            to = np.asarray(light) - pts
            d2 = (to * to).sum(-1)
            on_mesh = (to * n).sum(-1) / d2 ** 1.5
            ratio = on_mesh / sphere_irradiance(pts * (R / np.linalg.norm(pts, axis=-1, keepdims=True)), light)
            assert lo <= ratio.min() and ratio.max() <= hi
            # second order in the facet's size with the light at the centre, first order (the tilt of the normal) off it
            assert hi / lo - 1.0 < (0.005 / 4 ** (subdivisions - 4) if light == CENTRE else 0.06 / 2 ** (subdivisions - 4))
    # the area average of the direct lighting is I / R^2 wherever the light is (all of its flux lands on the sphere)
    z = (np.arange(20000) + 0.5) / 10000.0 - 1.0
    ring = R * np.stack([np.sqrt(1.0 - z * z), np.zeros_like(z), z], -1)
    assert abs(sphere_irradiance(ring, OFF_CENTRE).mean() * R ** 2 - 1.0) < 1e-6


# ---------------------------------------------------------------------------------------------------------------------
# the oracle
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle_scene(subdivisions, light_pos, albedo, flat=True):
    return OracleScene(sphere_room(subdivisions, light_pos, albedo, flat))


def render_oracle(scene, n, launches, depth, seed=3):
    o = OracleRenderer(scene, n, n)
    o.set_integrator(abi.PATH_TRACE)
    o.set_depth(depth)
    o.set_seed(seed)
    o.step(launches)
    return o.read_hdr()


@ALL
def test_oracle_enclosure_matches_the_closed_form(key):
    ref = reference(*key, CPU_FRAME)
    ref.check_power(CASES[key][1])
    ref.check(render_oracle(oracle_scene(ref.subdivisions, key[0], key[1]), CPU_FRAME, LAUNCHES, key[2]))


def test_oracle_smooth_sphere_is_not_brighter_than_the_flat_closed_form():
    """With smooth normals a sampled direction can leave the mesh and end the path: the image can only lose light.  One-sided."""
    key = (CENTRE, 252, 6)
    ref = reference(*key, CPU_FRAME)
    img = render_oracle(oracle_scene(ref.subdivisions, key[0], key[1], flat=False), CPU_FRAME, LAUNCHES, key[2])
    got = (img[..., :3].astype(np.float64) / img[..., 3:4]).mean(axis=(0, 1))
    assert (img[..., 3] == LAUNCHES).all() and (got > 0.9 * ref.interval()[0]).all()
    assert (got <= ref.interval()[1]).all(), (got, ref.interval()[1])


# ---------------------------------------------------------------------------------------------------------------------
# the HIP path
# ---------------------------------------------------------------------------------------------------------------------
def render_hip(instance, desc, n, launches, depth, mode, seed=3, node_width=None, chains=None, as_levels=None):
    if as_levels:
        instance.set_as_levels(as_levels)
    try:
        scene = glaze_amd.RayTraceScene.from_desc(instance, desc)
    finally:
        instance.set_as_levels("auto")
    if as_levels:
        assert scene.info().as_levels == {"flat": 1, "two_level": 2}[as_levels]
    r = glaze_amd.RayTraceRenderer.new(instance, scene, n, n)
    r.set_integrator(glaze_amd.Integrator.PATH_TRACE)
    r.set_launch_mode(mode)
    assert r.launch_mode() == mode
    if node_width:
        r.set_node_width(node_width)
        assert r.node_width() == node_width
    if chains:
        r.set_chains(chains)
    r.set_depth(depth)
    r.set_seed(seed)
    r.step(launches)
    return r.read_hdr()


MODES = pytest.mark.parametrize("mode", ["two_kernels", "path"])


@pytest.mark.gpu
@MODES
@ALL
def test_hip_enclosure_matches_the_closed_form(instance, key, mode):
    ref = reference(*key, GPU_FRAME)
    ref.check_power(CASES[key][1])
    ref.check(render_hip(instance, sphere_room(ref.subdivisions, key[0], key[1]), GPU_FRAME, LAUNCHES, key[2], mode))


@pytest.mark.gpu
@pytest.mark.parametrize("variant,mode", [("node_width_8", "two_kernels"), ("node_width_8", "path"), ("two_level", "two_kernels"),
                                          ("chains_3", "two_kernels"), ("chains_3", "path")])
def test_hip_enclosure_in_the_other_launch_shapes(instance, variant, mode):
    """the 8-wide walk, the two-level walk (the sphere split into 8 instanced meshes; a two-level scene always runs as two kernels) and
    three concurrent launch chains"""
    key = (CENTRE, 150, 6)
    ref = reference(*key, GPU_FRAME)
    ref.check_power(CASES[key][1])
    kw = {"node_width_8": dict(node_width=8), "two_level": dict(as_levels="two_level"), "chains_3": dict(chains=3)}[variant]
    desc = sphere_room(ref.subdivisions, key[0], key[1], parts=8 if variant == "two_level" else 1)
    ref.check(render_hip(instance, desc, GPU_FRAME, LAUNCHES, key[2], mode, **kw))


@pytest.mark.gpu
@MODES
@pytest.mark.parametrize("depth", [6, 12])
@pytest.mark.parametrize("flat", [True, False], ids=["flat", "smooth"])
def test_hip_enclosure_parity_with_the_oracle(instance, flat, depth, mode):
    """HIP against the oracle.  The smooth sphere is the first scene of the suite whose rays leave a closed mesh from the inside."""
    from test_gpu_render import assert_parity, render_both
    desc = sphere_room(4, CENTRE, 252, flat=flat)
    r, o, _ = render_both(instance, desc, 48, 48, spp=16, depth=depth, seed=11)
    assert r.steps_per_sample() == depth                                   # a path has depth + 1 vertices: samples and camera rays drift apart
    assert_parity(r, o, "sphere flat=%s depth %d (auto mode)" % (flat, depth))
    r2 = glaze_amd.RayTraceRenderer.new(instance, glaze_amd.RayTraceScene.from_desc(instance, desc), 48, 48)
    r2.set_launch_mode(mode)
    assert r2.launch_mode() == mode
    r2.set_depth(depth)
    r2.set_seed(11)
    r2.step(16 * depth)
    assert_parity(r2, o, "sphere flat=%s depth %d %s" % (flat, depth, mode))


@pytest.mark.gpu
def test_hip_smooth_sphere_is_not_brighter_than_the_flat_closed_form(instance):
    key = (CENTRE, 252, 6)
    ref = reference(*key, GPU_FRAME)
    img = render_hip(instance, sphere_room(ref.subdivisions, key[0], key[1], flat=False), GPU_FRAME, LAUNCHES, key[2], "two_kernels")
    got = (img[..., :3].astype(np.float64) / img[..., 3:4]).mean(axis=(0, 1))
    assert (img[..., 3] == LAUNCHES).all() and (got > 0.9 * ref.interval()[0]).all()
    assert (got <= ref.interval()[1]).all(), (got, ref.interval()[1])
