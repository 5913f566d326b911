"""References for the traversal tests: a float64 brute-force ray tracer, and lower bounds on a ray's traversal stack computed from a
read-back node array (what proves that a test drove a tracer's stack past its LDS levels: there is no device counter)."""
import numpy as np

EMPTY_CHILD = 0x7FFFFFFF        # kBvhEmptyChild; links < 0 are leaves, the others inner nodes (numbers in the same array)


def _links(nodes, width):
    nodes = np.asarray(nodes)
    if width not in (4, 8) or nodes.ndim != 2 or nodes.shape[1] != 4 * width:
        raise ValueError("width 4 takes (n, 16) nodes, width 8 (n, 32)")
    return np.ascontiguousarray(nodes[:, 3 * width:]).view(np.int32).astype(np.int64)


def min_first_leaf_stack(nodes, width, root=0):
    """The minimum over all leaves below `root` of the sum of (children - 1) along the root-to-leaf path.

    A visit of a node whose child boxes the ray all overlaps enters one child and pushes the others, so a ray that overlaps EVERY box
    holds exactly that sum on its stack when it reaches its first leaf, whichever child each visit enters first: the minimum is a lower
    bound on the peak depth of such a ray's stack under any visit order (nearest first and farthest first alike)."""
    links = _links(nodes, width)
    if links.shape[0] == 0:
        return 0
    best = None
    frontier, acc = np.array([root], np.int64), np.array([0], np.int64)
    visited = 0
    while frontier.size:
        visited += frontier.size
        if visited > links.shape[0]:
            raise ValueError("the links do not form a tree")
        ch = links[frontier]                                                   # (m, width)
        present = ch != EMPTY_CHILD
        below = (acc + present.sum(1) - 1)[:, None] + np.zeros_like(ch)
        leaf = present & (ch < 0)
        if leaf.any():
            low = int(below[leaf].min())
            best = low if best is None else min(best, low)
        inner = present & (ch >= 0)
        frontier, acc = ch[inner], below[inner]
    return best


def _z_bounds(nodes, width):
    """quantised (lo, hi) of every child box along z: one word per axis and child, lo | hi << 16, children 3 words apart"""
    w = np.asarray(nodes)[:, 2:3 * width:3].astype(np.int64)
    return w & 0xFFFF, w >> 16


def first_leaf_stack_along_z(nodes, width, direction, far_first, root=0):
    """Lower bound on the stack a ray along +z (direction +1) or -z (-1) holds at its first leaf when it starts outside the scene's
    bounds and overlaps every box, for a walk that enters the nearest child first (far_first False) or the farthest (True).

    The ray enters a box through its low z face (+z) or its high one (-z), so the child entered first is the one with the smallest low
    bound (+z nearest, -z farthest ... by the high bound) -- read off the quantised boxes the tracer itself tests.  Children that tie on
    that bound are all followed and the smaller result taken.  This is the bound for a chain (the comb), where min_first_leaf_stack is
    the root's own leaves whatever the chain's length: there the depth depends on the end the walk starts from."""
    links = _links(nodes, width)
    zlo, zhi = _z_bounds(nodes, width)
    key = zlo if direction > 0 else -zhi                                        # entry distance along the ray, up to a constant
    if far_first:
        key = -key

    def walk(node, acc):
        ch = links[node]
        present = ch != EMPTY_CHILD
        acc += int(present.sum()) - 1
        first = present & (key[node] == key[node][present].min())
        return min(acc if c < 0 else walk(int(c), acc) for c in ch[first])

    return walk(root, 0) if links.shape[0] else 0


# ---- float64 brute force ------------------------------------------------------------------------------------------------------------
EDGE = 1e-4          # a barycentric coordinate this close to 0 makes a candidate ambiguous between float32 and float64
NEAR = 1e-6          # relative distance in t within which two candidates, or a candidate and a limit, are not told apart


class Hits:
    """what brute_force found for one (tmin, tmax): t (float64, +inf for a miss) and tri (int64, -1 for a miss) of the closest hit in
    (tmin, tmax), ties to the smaller triangle number; any (bool): some hit in (tmin, tmax); keep (bool): False where float32 may
    rightly find another closest hit -- the best hit, or a candidate nearer than it or within NEAR of it in t, touches an edge within
    EDGE or lies within NEAR of tmin or tmax; keep_any (bool): the same for `any` -- no hit is beyond doubt and some candidate in
    range is in doubt"""

    def __init__(self, n):
        self.t, self.tri = np.full(n, np.inf), np.full(n, -1, np.int64)
        self.any, self.keep, self.keep_any = np.zeros(n, bool), np.ones(n, bool), np.ones(n, bool)

    def first(self, n):
        out = Hits(0)
        for name in ("t", "tri", "any", "keep", "keep_any"):
            setattr(out, name, getattr(self, name)[:n])
        return out


def brute_force(tris, o, d, limits, chunk=4):
    """Moeller-Trumbore in float64 of every ray against every triangle (tris: (T, 3, 3), world-triangle order), judged once per entry
    (tmin, tmax) of `limits` (tmax: None = unlimited, or one value per ray): a list of Hits.

    The determinants of the method, det = e1 . (d x e2), u det = (o - v0) . (d x e2), v det = d . ((o - v0) x e1) and
    t det = e2 . ((o - v0) x e1), are taken apart into products of one per-ray and one per-triangle vector (with m = o x d and
    n = e1 x e2: det = -d . n, u det = e2 . m - d . (e2 x v0), v det = -e1 . m - d . (v0 x e1), t det = (o - v0) . n), so that a
    block of rays meets all triangles in five matrix products.  What follows works on the candidates alone, the pairs whose
    barycentric coordinates are all above -EDGE."""
    tris = np.asarray(tris, np.float64)
    o, d = np.asarray(o, np.float32).astype(np.float64).reshape(-1, 3), np.asarray(d, np.float32).astype(np.float64).reshape(-1, 3)
    n, n_tris = o.shape[0], tris.shape[0]
    limits = [(float(lo), np.full(n, np.inf) if hi is None else np.broadcast_to(np.asarray(hi, np.float32).astype(np.float64), (n,))) for lo, hi in limits]
    v0, e1, e2 = tris[:, 0], tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0]
    normal = np.cross(e1, e2)
    e2_v0, v0_e1, v0_n = np.cross(e2, v0).T.copy(), np.cross(v0, e1).T.copy(), (v0 * normal).sum(-1)
    e1t, e2t, nt = e1.T.copy(), e2.T.copy(), normal.T.copy()
    out = [Hits(n) for _ in limits]
    for a in range(0, n, chunk):
        oo, dd = o[a:a + chunk], d[a:a + chunk]
        m = np.cross(oo, dd)
        with np.errstate(all="ignore"):
            inv = -1.0 / (dd @ nt)
            u = (m @ e2t - dd @ e2_v0) * inv
            v = (-(m @ e1t) - dd @ v0_e1) * inv
            low = np.minimum(np.minimum(u, v), 1.0 - u - v)
            row, col = np.nonzero(low > -EDGE)                                  # (NaN, a ray in the triangle's plane, is no candidate)
            low = low[row, col]
            t = ((oo @ nt)[row, col] - v0_n[col]) * inv[row, col]
        for (tmin, tmax), h in zip(limits, out):
            far = tmax[a:a + chunk][row]
            inside = (t > tmin) & (t < far)
            hit = (low >= 0.0) & inside
            at_limit = ((t >= tmin * (1 - NEAR)) & (t <= tmin * (1 + NEAR))) | ((t >= far * (1 - NEAR)) & (t <= far * (1 + NEAR)))
            touchy = ((low < EDGE) & inside) | at_limit                         # candidates float32 may see differently
            best = np.full(oo.shape[0], np.inf)
            np.minimum.at(best, row[hit], t[hit])
            first = hit & (t == best[row])
            tri = np.full(oo.shape[0], n_tris, np.int64)
            np.minimum.at(tri, row[first], col[first])                          # ties: the smallest triangle number
            found = np.isfinite(best)
            h.t[a:a + chunk], h.tri[a:a + chunk], h.any[a:a + chunk] = best, np.where(found, tri, -1), found
            doubt = touchy & (t <= (best * (1 + NEAR))[row])
            h.keep[a:a + chunk] = np.bincount(row[doubt], minlength=oo.shape[0]) == 0
            # "some hit" stands when one hit is beyond doubt, wherever along the ray; otherwise no candidate may be in doubt
            sure = np.bincount(row[hit & ~touchy], minlength=oo.shape[0]) > 0
            h.keep_any[a:a + chunk] = sure | (np.bincount(row[touchy], minlength=oo.shape[0]) == 0)
    return out




TMIN_CLOSEST, TMIN_ANY = 1e-4, 1e-3      # the trace hooks' defaults
MAX_DROPPED = 0.01                       # of a ray set; a condition on the chosen seeds, not a measurement
T_TOLERANCE = 1e-5                       # relative, float32 tracer against float64


class RayCase:
    """A scene description, a ray set against it and the brute-force answers, made once and shared: closest hits, and any-hit under each
    of the ray set's limits.  Every prefix of the ray set is a ray set of its own (the kinds of rays are interleaved)."""

    def __init__(self, desc, rays):
        from stack_scenes import world_triangles
        self.desc = desc
        self.o, self.d, self.tmax = rays
        self.n = self.o.shape[0]
        tris, self.inst_of_tri = world_triangles(desc)
        self.closest, *self.any = brute_force(tris, self.o, self.d, [(TMIN_CLOSEST, None)] + [(TMIN_ANY, tm) for tm in self.tmax])

    def dropped(self, n=None):
        """the largest share of the first n rays that one of the comparisons leaves out"""
        n = self.n if n is None else n
        return max(float((~k[:n]).mean()) for k in [self.closest.keep] + [a.keep_any for a in self.any])

    def check_closest(self, t, tri, inst, n=None):
        """t, tri, inst: a float32 tracer's closest hits of the first n rays (tri: world triangle, 0xFFFFFFFF and t = inf for a miss)"""
        n = self.n if n is None else n
        ref = self.closest.first(n)
        assert t.shape == (n,) and (~ref.keep).sum() <= MAX_DROPPED * n
        got_tri = np.where(np.isfinite(t), tri.astype(np.int64), -1)
        got_inst = np.where(np.isfinite(t), inst.astype(np.int64), -1)
        want_inst = np.where(ref.tri >= 0, self.inst_of_tri[np.maximum(ref.tri, 0)], -1)
        wrong = ref.keep & ((got_tri != ref.tri) | (got_inst != want_inst))
        assert not wrong.any(), "%d of %d rays hit another triangle than the brute force, first ray %d: %d against %d" % (
            wrong.sum(), n, np.argmax(wrong), got_tri[np.argmax(wrong)], ref.tri[np.argmax(wrong)])
        both = ref.keep & (ref.tri >= 0)
        rel = np.abs(t[both].astype(np.float64) - ref.t[both]) / ref.t[both]
        assert rel.size == 0 or rel.max() <= T_TOLERANCE, "t off by %.3g relative" % rel.max()

    def check_any(self, which, out, n=None):
        n = self.n if n is None else n
        ref = self.any[which].first(n)
        assert out.shape == (n,) and (~ref.keep_any).sum() <= MAX_DROPPED * n
        wrong = ref.keep_any & (out.astype(bool) != ref.any)
        assert not wrong.any(), "%d of %d any-hit answers differ from the brute force, first ray %d" % (wrong.sum(), n, np.argmax(wrong))
