"""Scenes and ray sets that force deep traversal stacks (plain numpy; tests/test_gpu_stack_spill.py, tests/test_stack_scenes.py).

Deck: n thin cards stacked along z.  A card is a parallelogram strip along the diagonal of the square [-1, 1]^2, cut into two triangles
in fan order (a, b, c), (a, c, d): its box is the whole square while most of the square is empty, so a ray along z at a point off the
strips passes through every box of the hierarchy and hits nothing, and a ray on all of them hits the nearest card.  One edge of the
strip is jittered per card (fixed seed) between two corners that stay, so that in a band next to the strips a ray passes some cards and
hits a later one; a few cards lie exactly on top of their predecessor (equal t: the smaller world triangle id wins).

Comb: a few dozen cards at geometrically growing z.  Every builder makes a chain of it -- each level one inner child and leaves beside
it -- so the stack of a ray that enters the inner child first grows with every level while the scene stays a few hundred triangles.
"""
import numpy as np

from glaze_amd import abi
from glaze_amd.scene_desc import INSTANCE_DTYPE, MESH_DTYPE, VERTEX_DTYPE, SceneDesc, make_camera, make_light, make_material, make_meta
from glaze_amd.scenes import checker_texture

HALF = 0.15              # every card's box is [-1 - HALF, 1 + HALF] x [-1, 1]: its corners a and c do not move
UPPER = (-0.05, 0.15)    # the strip's upper edge u, drawn per card: on y = -1 the card covers -HALF < x - y < u, on y = +1 -u < x - y < HALF
SPAN = 0.8               # rays along z keep |x|, |y| <= SPAN: inside every card's box
COINCIDENT_EVERY = 128   # card k with k % 128 == 51 lies exactly on card k - 1 (its sibling in a balanced hierarchy)
Z_UNIT = 2.0 ** -22      # exact in float32 anywhere in [-1, 1]


def _upper_edges(rng, n):
    """The jitter moves the strip's corners b and d (its place across the square and its slant at once, cover_threshold below) and
    leaves the box, spanned by a and c, alone: boxes whose centres or
    footprints followed the jitter would have the LBVH and PLOC builders sort, and the SAH builder and the wide collapse weigh, the
    jitter instead of the stacking."""
    u = rng.uniform(UPPER[0], UPPER[1], n).astype(np.float32)
    # the two end cards are the narrowest: a ray of the band passes the card it meets first and hits one of the next few, the cards
    # whose entries lie at the very top of its stack when it reaches that first leaf
    u[0] = u[-1] = UPPER[0]
    return u


def deck_cards(n, seed=5):
    """(z, u) of the n cards (n a power of two): z ascending from -1 in steps of 2 / n, u the strip's upper edge.  Every height is
    pushed up by a random multiple of Z_UNIT, a thirty-second of a step at most: it leaves each card in its own 1 / n of the range
    (the hierarchy LBVH and binned SAH build stays the balanced one) and gives PLOC, which merges mutually nearest neighbours, gaps
    that differ (among equal gaps it merges one pair a round, into a hierarchy thousands of levels deep).  The last card stands half
    a step higher, so that the cards' places in the range of their centres keep clear of the cell borders of a power-of-two grid."""
    rng = np.random.default_rng(seed)
    step = 2.0 / n
    push = rng.integers(0, max(1, int(step / 32 / Z_UNIT)) + 1, n) * Z_UNIT
    push[0] = 0.0
    z = -1.0 + step * np.arange(n) + push
    z[-1] = 1.0 - step / 2
    u = _upper_edges(rng, n)
    twin = np.flatnonzero(np.arange(n) % COINCIDENT_EVERY == 51)
    z[twin], u[twin] = z[twin - 1], u[twin - 1]
    assert np.array_equal(z.astype(np.float32).astype(np.float64), z)
    return z.astype(np.float32), u


def comb_cards(n=36, ratio=1.5, seed=6):
    """(z, u) of the comb's cards: z = 16 ratio^k, so that from the first gap on a subtree's extent along z outweighs its footprint
    in its box area (the SAH builder then cuts one card off the far end at a time instead of halving the near ones)"""
    rng = np.random.default_rng(seed)
    z = (16.0 * ratio ** np.arange(n)).astype(np.float32)
    u = _upper_edges(rng, n)
    z[7], u[7] = z[6], u[6]                                      # one coincident pair
    return z, u


def card_corners(z, u, shift_x=None):
    """(n, 4, 3) float32: the corners a, b, c, d of every card (a, b on y = -1, c, d on y = +1); shift_x moves card k by shift_x[k] in x"""
    z, u = np.asarray(z, np.float32), np.asarray(u, np.float32)
    sx = np.zeros_like(z) if shift_x is None else np.asarray(shift_x, np.float32)
    one, width = np.ones_like(z), u + np.float32(HALF)
    a = np.stack([sx - 1 - np.float32(HALF), -one, z], -1)
    b = np.stack([sx - 1 - np.float32(HALF) + width, -one, z], -1)
    c = np.stack([sx + 1 + np.float32(HALF), one, z], -1)
    d = np.stack([sx + 1 + np.float32(HALF) - width, one, z], -1)
    return np.stack([a, b, c, d], 1).astype(np.float32)


def card_mesh(corners, paired=True):
    """vertices (VERTEX_DTYPE) and indices of the cards: four shared vertices a card (its two triangles pair into one leaf), or three
    private ones a triangle (nothing pairs); the triangles, their order and their vertex order are the same either way"""
    n = corners.shape[0]
    fan = np.array([0, 1, 2, 0, 2, 3])
    uv = np.array([[0, 0], [1, 0], [1, 1], [0, 1]], np.float32)
    if paired:
        pos, tex = corners.reshape(-1, 3), np.tile(uv, (n, 1))
        indices = (4 * np.arange(n)[:, None] + fan[None, :]).reshape(-1)
    else:
        pos, tex = corners[:, fan].reshape(-1, 3), np.tile(uv[fan], (n, 1))
        indices = np.arange(6 * n)
    v = np.zeros(pos.shape[0], VERTEX_DTYPE)
    v["vv"], v["vn"], v["vt"] = pos, (0.0, 0.0, -1.0), tex
    return v, indices.astype(np.uint32)


def world_triangles(desc):
    """(T, 3, 3) float64 world-space triangles in world-triangle order (instance by instance, each its mesh's triangles in index order)
    and (T,) the instance of each"""
    pos = desc.vertices["vv"].astype(np.float64)
    meshes = {int(m["id"]): m for m in desc.meshes}
    tris, inst = [], []
    for i, ins in enumerate(desc.instances):
        m = meshes[int(ins["mesh_id"])]
        idx = desc.indices[int(m["index_offset"]):int(m["index_offset"]) + int(m["index_count"])].reshape(-1, 3)
        # the device transforms in float32 (the oracle does too): the reference takes the float32 world vertices it would have got
        mat = desc.transforms[int(ins["transform_id"])].reshape(4, 4).T.astype(np.float64)
        p = pos[idx]
        if not np.array_equal(mat, np.eye(4)):
            p = (p @ mat[:3, :3].T + mat[:3, 3]).astype(np.float32).astype(np.float64)
        tris.append(p)
        inst.append(np.full(idx.shape[0], i, np.int64))
    return np.concatenate(tris), np.concatenate(inst)


def _surroundings(z_lo, z_hi, sun=True):
    """materials, textures, lights, camera and meta for a stack of cards between z_lo and z_hi: the camera looks along the stack from in
    front of it (its frame stays inside the cards' square all the way through), one lamp beside the camera, and a sun and a lamp BEHIND
    the stack, so that shadow rays cross it from the near end to the far end"""
    depth = float(z_hi - z_lo)
    materials = [make_material("default"), make_material("card", mtype=abi.MAT_LAMBERT, diffuse=1, diffuse_mul=(230, 220, 200)),
                 make_material("mirror", mtype=abi.MAT_MIRROR)]
    textures = [(abi.TEX_RGBA_SRGB, np.full((1, 1, 4), 255, np.uint8), "default"), (abi.TEX_RGBA_SRGB, checker_texture(32, 8, 120, 240), "checker")]
    lights = [make_light(abi.LIGHT_OMNI, "front lamp", position=(0.3, 0.2, z_lo - 0.5 * depth), intensity=3.0 * depth * depth),
              make_light(abi.LIGHT_OMNI, "back lamp", position=(0.45, -0.1, z_hi + 0.25 * depth), intensity=8.0 * depth * depth)]
    if sun:
        lights.append(make_light(abi.LIGHT_SUN, "sun behind", direction=(-0.12, 0.05, -1.0), intensity=2.0))
    # half-width SPAN at the far end: tan(fovx / 2) = SPAN / (2 depth) from one depth in front of the stack
    camera = make_camera(position=(0, 0, z_lo - depth), target=(0, 0, z_hi), up=(0, 1, 0), fovx=np.float32(2.0 * np.arctan(SPAN / (2.0 * depth))),
                         near=1e-3 * depth, far=100.0 * depth)
    meta = make_meta(centre=(0, 0, 0.5 * (z_lo + z_hi)), radius=float(max(depth, 2.0)), exposure=1.0)
    return materials, textures, lights, camera, meta


def cards_scene(z, u, paired=True, shift_x=None):
    """one mesh of all cards, one instance"""
    v, idx = card_mesh(card_corners(z, u, shift_x), paired)
    materials, textures, lights, camera, meta = _surroundings(float(np.min(z)), float(np.max(z)))
    return SceneDesc(v, idx, np.array([(0, 1, 0, idx.size)], MESH_DTYPE), None, np.array([(0, 0)], INSTANCE_DTYPE), materials, lights, textures,
                     camera, meta)


def deck_scene(n, paired=True, seed=5):
    return cards_scene(*deck_cards(n, seed), paired=paired)


def comb_scene(n=36, paired=True):
    return cards_scene(*comb_cards(n), paired=paired)


SPREAD_STEP = 4.0        # spread_shift: card k stands SPREAD_STEP * k to the right of its place in the deck


def spread_shift(n):
    """(the last card half a step further, like its height in deck_cards)"""
    shift = SPREAD_STEP * np.arange(n)
    shift[-1] += SPREAD_STEP / 2
    return shift.astype(np.float32)


def translation(x=0.0, y=0.0, z=0.0):
    m = np.eye(4, dtype=np.float32)
    m[:3, 3] = (x, y, z)
    return m.T.reshape(16)                                       # column-major


def instanced_deck_scene(n, offsets, paired=True, seed=5):
    """the deck as ONE mesh under len(offsets) instances, instance i translated by offsets[i] (x, y, z)"""
    z, u = deck_cards(n, seed)
    v, idx = card_mesh(card_corners(z, u), paired)
    materials, textures, lights, camera, meta = _surroundings(-1.0, 1.0)
    transforms = np.stack([translation(*o) for o in offsets])
    instances = np.array([(0, i) for i in range(len(offsets))], INSTANCE_DTYPE)
    return SceneDesc(v, idx, np.array([(0, 1, 0, idx.size)], MESH_DTYPE), transforms, instances, materials, lights, textures, camera, meta)


def mirror_deck_scene(n, seed=5):
    """the deck with its FIRST card a mirror (a mesh and an instance of its own) and the others behind it, the LAST of them a mirror
    that fills its whole box: a ray off the strips crosses every box, is reflected and crosses them all again on its way back.  Boxes,
    and with them the hierarchy, are the plain deck's."""
    z, u = deck_cards(n, seed)
    corners = card_corners(z, u)
    corners[-1, 1, 0], corners[-1, 3, 0] = corners[-1, 2, 0], corners[-1, 0, 0]      # b below c, d above a: the whole rectangle
    parts = [card_mesh(corners[:1]), card_mesh(corners[1:-1]), card_mesh(corners[-1:])]
    vertices = np.concatenate([v for v, _ in parts])
    first = np.cumsum([0] + [v.size for v, _ in parts])
    indices = np.concatenate([i + first[k] for k, (_, i) in enumerate(parts)])
    start = np.cumsum([0] + [i.size for _, i in parts])
    meshes = np.array([(k, material, start[k], parts[k][1].size) for k, material in enumerate((2, 1, 2))], MESH_DTYPE)
    materials, textures, lights, camera, meta = _surroundings(float(z.min()), float(z.max()))
    return SceneDesc(vertices, indices, meshes, None, np.array([(0, 0), (1, 0), (2, 0)], INSTANCE_DTYPE), materials, lights, textures, camera, meta)


# ---- rays -------------------------------------------------------------------------------------------------------------------------
# The kinds of ray, in the order they are dealt (ray i is of kind KINDS[i % len(KINDS)]).  The first two come first on purpose: of all
# kinds they depend most on the entries at the TOP of a deep stack -- the hit is one of the few cards next to the first leaf.
KINDS = ("band +z",        # full span, in the band where only some cards are hit: passes a few cards and hits one of the next
         "band -z",
         "off +z",         # full span, off every strip: misses everything, visits every leaf
         "on -z",          # full span, on every strip: hits the last card
         "between +z",     # from between two random cards, in the band
         "off -z",
         "on +z",          # hits the first card
         "between -z",
         "tilted +z",      # from on the strips in front of the stack to off the strips behind it: leaves them part-way
         "tilted -z")
N_KINDS = len(KINDS)
RAY_COUNTS = (1, 2, 63, 64, 65, 257, 2049)


def kinds_of(n):
    return np.array(KINDS)[np.arange(n) % N_KINDS]


def cover_threshold(x, y):
    """a card with upper edge u covers the point (x, y) of its plane exactly when u > cover_threshold(x, y): the strip's long edges run
    from (-1 - HALF, -1) to (1 - u, 1) and from (-1 + u, -1) to (1 + HALF, 1)"""
    g, lam = x - y, (y + 1.0) / 2.0
    with np.errstate(all="ignore"):
        return np.maximum((g - lam * HALF) / (1.0 - lam), HALF - (g + HALF) / lam)


def _points(rng, n, lo, hi):
    """n points of [-SPAN, SPAN]^2 with lo < cover_threshold < hi (drawn uniformly and sorted out)"""
    xs, ys = np.zeros(0), np.zeros(0)
    while xs.size < n:
        x, y = rng.uniform(-SPAN, SPAN, 64 * n + 1024), rng.uniform(-SPAN, SPAN, 64 * n + 1024)
        t = cover_threshold(x, y)
        keep = (t > lo) & (t < hi)
        xs, ys = np.concatenate([xs, x[keep]]), np.concatenate([ys, y[keep]])
    return xs[:n], ys[:n]


def stack_rays(z, n, seed):
    """n rays against a stack of cards at heights z (ascending), of the kinds above INTERLEAVED, so that neighbouring lanes of a wave
    push different entries.  Returns origins, directions (float32) and (tmax_far, tmax_mid): any-hit limits beyond the stack, and
    ending between two cards."""
    rng = np.random.default_rng(seed)
    z = np.asarray(z, np.float64)
    lo, hi = float(z.min()), float(z.max())
    depth = hi - lo
    kind = kinds_of(n)
    o, d = np.zeros((n, 3)), np.zeros((n, 3))
    x_off, y_off = _points(rng, n, UPPER[1] + 0.05, np.inf)      # under no card
    x_on, y_on = _points(rng, n, -np.inf, UPPER[0] - 0.01)       # under every card
    x_band, y_band = _points(rng, n, UPPER[0], UPPER[1] - 0.01)  # under some
    k = rng.integers(0, z.size - 1, n)
    between = z[k] + 0.37 * (z[np.minimum(k + 1, z.size - 1)] - z[k])
    before, behind = lo - 0.5 * depth, hi + 0.5 * depth
    up = np.char.endswith(kind, "+z")
    for name, (x, y) in {"band": (x_band, y_band), "off": (x_off, y_off), "on": (x_on, y_on), "between": (x_band, y_band)}.items():
        m = np.char.startswith(kind, name)
        o[m, 0], o[m, 1] = x[m], y[m]
        o[m, 2] = between[m] if name == "between" else np.where(up[m], before, behind)
        d[m, 2] = np.where(up[m], 1.0, -1.0)
    m = np.char.startswith(kind, "tilted")
    o[m] = np.stack([x_on[m], y_on[m], np.where(up[m], before, behind)], -1)
    to = np.stack([x_off[m], y_off[m], np.where(up[m], behind, before)], -1) - o[m]
    d[m] = to / np.linalg.norm(to, axis=1, keepdims=True)
    o, d = o.astype(np.float32), d.astype(np.float32)
    tmax_far = np.full(n, 4.0 * depth, np.float32)
    # ... and a limit that ends between two cards: 0.45 of a gap past the first card ahead of the ray, or the second ... fifth (where a
    # ray of the band finds its hit)
    levels = np.unique(z)
    oz = o[:, 2].astype(np.float64)
    ahead = np.where(up, np.searchsorted(levels, oz, "right"), np.searchsorted(levels, oz, "left") - 1)
    j = np.clip(ahead + np.where(up, 1, -1) * rng.integers(0, 5, n), 1, levels.size - 2)
    def stop_at(j):
        return np.where(up, levels[j] + 0.45 * (levels[j + 1] - levels[j]), levels[j] - 0.45 * (levels[j] - levels[j - 1]))

    # float32 must be able to tell the limit from the cards on either side of it: 0.45 of the gap at least 8e-6 of the distance (where
    # the gaps grow with z, the comb, a limit too far from its ray's origin for that moves up to where they are wide enough)
    for _ in range(levels.size):
        stop = stop_at(j)
        gap = np.where(up, levels[j + 1] - levels[j], levels[j] - levels[j - 1])
        j = np.where(0.45 * gap >= 8e-6 * np.abs(stop - oz), j, np.minimum(j + 1, levels.size - 2))
    stop = stop_at(j)
    along = (stop - oz) / d[:, 2].astype(np.float64)
    tmax_mid = np.where(along > 0, along, 0.5 * depth).astype(np.float32)
    return o, d, (tmax_far, tmax_mid)
