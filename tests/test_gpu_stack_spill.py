"""Every tracer's traversal stack driven past its LDS levels (kTraversalLdsStack = 17 for the 4-wide and the two-level walk,
GLZ_TRACE8_STACK = 28 for the 8-wide one) into the per-lane HBM spill area, in every place that allocates one: the trace hooks, the
renderer's chains, the first-hit pass and the guide chain that reuses its slots -- also after update_vertices, update_transforms and
change_scene, and in waves of a handful of rays, whose idle lanes steal from the LDS bottoms of stacks whose tops are in HBM.

There is no device counter.  What proves that a case spilled is a bound computed from the node array the case read back
(tests/trace_ref.py): min_first_leaf_stack, the least any ray that overlaps every box can have on its stack when it reaches its first
leaf, whatever the visit order.  Every deck case asserts that it is at least the tracer's LDS levels + 4, with one exception, stated
where it is made (PLOC over paired leaves).  A chain (the comb) has leaves next to its root, so that minimum is 3 whatever the chain's
length; there the depth depends on the end the walk starts from, and the comb cases assert first_leaf_stack_along_z for the rays that
enter the chain's inner child first (+z closest-hit rays, -z any-hit rays, which walk farthest first).  The scenes are
tests/stack_scenes.py; hits are held to a float64 brute force and, bit for bit, to the oracle.

Cards chosen -- the smallest power of 4 at which the bound holds for that builder -- and the bound reached (needed: 21 four wide, 32
eight wide).  The balanced hierarchy of 4^7 cards is 7 levels of 4-wide nodes with four children each, 7 x 3 = 21 exactly:

    scene, walk                          lbvh            ploc                         sah
    deck, 4-wide, paired leaves          4^7: 21         4^8: 19 (along z: 21)        4^7: 21
    deck, 4-wide, unpaired leaves        4^7: 21         4^8: 21                      4^7: 21
    deck, 8-wide (renders)               -               -                            4^8: 36 (4^7: 31)
    deck as one mesh, two instances      -               -                            4^7: 21 + 1 (top level)
    spread cards refitted into the deck  4^7: 21         -                            4^7: 21
    comb of 36, paired: +z near, -z far  22, 24          22, 24                       19, 21
    comb of 36, unpaired                 24, 25          24, 25                       21, 22
"""
import functools

import numpy as np
import pytest

import glaze_amd
from glaze_amd import distributed
from glaze_amd.scenes import cube_scene
from oracle.pyoracle import OracleRenderer, OracleScene, launch_constants

import stack_scenes as ss
from trace_ref import RayCase, first_leaf_stack_along_z, min_first_leaf_stack

pytestmark = pytest.mark.gpu

LDS_LEVELS_4, LDS_LEVELS_8 = 17, 28          # kTraversalLdsStack, GLZ_TRACE8_STACK (tests/test_stack_scenes.py holds them to the headers)
MARGIN = 4
NEED_4, NEED_8 = LDS_LEVELS_4 + MARGIN, LDS_LEVELS_8 + MARGIN
BUILDERS = ("lbvh", "ploc", "sah")
DECK_CARDS_4 = {"lbvh": 4 ** 7, "ploc": 4 ** 8, "sah": 4 ** 7}      # the table above
DECK_CARDS_8 = 4 ** 8
COMB_CARDS = 36
RAY_SEED = 15                                 # tests/test_stack_scenes.py: the brute force keeps 99 % of these ray sets and more
W, H = 130, 20                                # three 64 x 64 tiles, the last one two pixels wide: chains and ranks all own pixels
LAUNCHES = 6                                  # 2 samples at depth 3


def bits(a):
    return np.nan_to_num(np.asarray(a, np.float32), nan=-1.0).view(np.uint32)


def make_scene(desc, builder="auto", levels="flat"):
    """a scene on an instance of its own: the builder and the level count are the instance's settings"""
    inst = glaze_amd.RayTraceInstance.new()
    assert inst is not None
    inst.set_bvh_builder(builder)
    inst.set_as_levels(levels)
    scene = glaze_amd.RayTraceScene.from_desc(inst, desc)
    assert scene.info().as_levels == (2 if levels == "two_level" else 1)
    return scene


def two_level_bound(scene):
    """top level + mesh level of a two-level scene whose instances share one mesh: an instance entry keeps the top level's entries below
    the mesh's (and an exit marker between them, not counted)"""
    nodes = scene.debug_bvh()[0]
    base = scene.debug_tlas_instances().reshape(-1, 192)[:, 88:92].copy().view(np.uint32).ravel()      # TlasInstance::node_base
    assert (base == base[0]).all() and base[0] >= 1
    return min_first_leaf_stack(nodes[:base[0]], 4) + min_first_leaf_stack(nodes[base[0]:], 4)


# ---- what the cases share: descriptions, brute-force answers and the oracle's, made once -------------------------------------------
@functools.lru_cache(maxsize=None)
def cards(family, n):
    return ss.deck_cards(n) if family == "deck" else ss.comb_cards(n)


@functools.lru_cache(maxsize=None)
def description(family, n, paired=True):
    return ss.cards_scene(*cards(family, n), paired=paired)


class Answers:
    """a ray set against a description: the brute force's answers (RayCase) and the oracle's"""

    def __init__(self, desc, rays):
        self.case = RayCase(desc, rays)
        self.orc = OracleScene(desc)
        c = self.case
        self.closest = self.orc.trace_closest(c.o, c.d, 1e-4)
        self.any = [self.orc.trace_any(c.o, c.d, tm) for tm in c.tmax]

    def check(self, scene, counts, what):
        """the trace hooks of `scene` on the first n rays, for every n of counts"""
        c = self.case
        for n in counts:
            got = scene.debug_trace_closest(c.o[:n], c.d[:n], 1e-4)
            for g, want in zip(got, self.closest):
                assert np.array_equal(bits(g) if g.dtype == np.float32 else g, bits(want[:n]) if want.dtype == np.float32 else want[:n]), \
                    "%s, %d rays: closest hits differ from the oracle's" % (what, n)
            c.check_closest(got[0], got[1], got[2], n)
            for which, tm in enumerate(c.tmax):
                hit = scene.debug_trace_any(c.o[:n], c.d[:n], tm[:n])
                assert np.array_equal(hit, self.any[which][:n]), "%s, %d rays, limit %d: any-hit answers differ from the oracle's" % (what, n, which)
                c.check_any(which, hit, n)
        # the ray set does what it is for: rays that miss everything, rays that hit, limits that decide
        assert 0.2 < np.isfinite(self.closest[0]).mean() < 0.9 and self.any[0].mean() > self.any[1].mean() + 0.01


def ray_counts(n):
    """1 ... 257 rays and a few thousand; against 4^8 cards a few hundred, to keep the brute force to seconds"""
    return ss.RAY_COUNTS if n <= 4 ** 7 else ss.RAY_COUNTS[:-1] + (513,)


@functools.lru_cache(maxsize=None)
def answers(family, n):
    """(the triangles and their order do not depend on how the vertices are shared: one set of answers serves paired and unpaired leaves)"""
    return Answers(description(family, n), ss.stack_rays(cards(family, n)[0], ray_counts(n)[-1], RAY_SEED))


@functools.lru_cache(maxsize=None)
def oracle_render(family, n, tiles=()):
    o = OracleRenderer(answers(family, n).orc, W, H)
    o.set_depth(3)
    o.set_seed(7)
    if tiles:
        o.set_tiles(list(tiles))
    o.step(LAUNCHES)
    return o.read_hdr()


def render(r, mode="auto", width=0, chains=0, partition=(0, 1)):
    r.set_launch_mode(mode)
    r.set_node_width(width)
    r.set_chains(chains)
    r.set_partition(*partition)
    r.set_depth(3)
    r.set_seed(7)
    r.restart()
    r.step(LAUNCHES)
    return r.read_hdr()


# ---- the trace hooks ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("paired", [True, False], ids=["paired", "unpaired"])
@pytest.mark.parametrize("builder", BUILDERS)
def test_trace_hooks_on_the_deck(builder, paired):
    n = DECK_CARDS_4[builder]
    scene = make_scene(description("deck", n, paired), builder)
    bound = min_first_leaf_stack(scene.debug_bvh()[0], 4)
    along = [first_leaf_stack_along_z(scene.debug_bvh()[0], 4, dr, far) for dr in (1, -1) for far in (False, True)]
    print("deck of %d, %s, %s: min_first_leaf_stack %d, along z %s, depth %d" % (n, builder, "paired" if paired else "unpaired", bound, along, scene.info().bvh_depth))
    if builder == "ploc" and paired:
        # PLOC's agglomerative hierarchy of the paired deck leaves some cards two levels from the root whatever their number (the
        # minimum is 15, 16, 19 at 4^6, 4^7, 4^8 cards): no power of 4 up to 65 536 reaches the bound over ALL leaves.  What it does
        # reach is the bound for the rays of this ray set that run along z and overlap every box -- from either end, nearest child
        # first or farthest first -- which is what this one case asserts
        assert min(along) >= NEED_4
    else:
        assert bound >= NEED_4
    links = scene.debug_bvh()[0][:, 12:16].view(np.int32)
    assert ((links < 0).sum() == n) == paired                     # a card is one leaf, or its two triangles are one each
    answers("deck", n).check(scene, ray_counts(n), "deck, %s" % builder)


@pytest.mark.parametrize("paired", [True, False], ids=["paired", "unpaired"])
@pytest.mark.parametrize("builder", BUILDERS)
def test_trace_hooks_on_the_comb(builder, paired):
    scene = make_scene(description("comb", COMB_CARDS, paired), builder)
    nodes = scene.debug_bvh()[0]
    near, far = first_leaf_stack_along_z(nodes, 4, +1, False), first_leaf_stack_along_z(nodes, 4, -1, True)
    print("comb of %d, %s, %s: +z nearest first %d, -z farthest first %d, least of all leaves %d, depth %d" % (
        COMB_CARDS, builder, "paired" if paired else "unpaired", near, far, min_first_leaf_stack(nodes, 4), scene.info().bvh_depth))
    # How much of a chain the comb becomes is the builder's choice (binned SAH weighs a cut by the cards on either side and takes
    # several off the far end at a time): both kinds of ray must go past the LDS levels, the deeper kind by the full margin
    assert min(near, far) > LDS_LEVELS_4 and max(near, far) >= NEED_4
    answers("comb", COMB_CARDS).check(scene, ss.RAY_COUNTS, "comb, %s" % builder)


# ---- renders -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [4, 8])
def test_renders_of_the_deck_in_every_launch_shape(instance, width):
    """k_trace (its shadow pass walks farthest first, and the sun and a lamp stand BEHIND the deck), k_trace8 and k_path, one chain and
    three, one rank of three: bit for bit the oracle's image, and so each other's"""
    n = DECK_CARDS_4["sah"] if width == 4 else DECK_CARDS_8
    scene = glaze_amd.RayTraceScene.from_desc(instance, description("deck", n))
    bound4, bound8 = min_first_leaf_stack(scene.debug_bvh()[0], 4), min_first_leaf_stack(scene.debug_bvh8(), 8)
    print("deck of %d, default builder: min_first_leaf_stack %d (4-wide), %d (8-wide)" % (n, bound4, bound8))
    assert bound4 >= NEED_4 and (width == 4 or bound8 >= NEED_8)   # (k_path walks the 4-wide nodes at either setting)
    want = oracle_render("deck", n)
    assert (want[..., :3].sum(-1) > 0).mean() > 0.1 and (want[..., :3].sum(-1) == 0).mean() > 0.1     # lit cards, and rays that pass them all
    r = glaze_amd.RayTraceRenderer.new(instance, scene, W, H)
    images = {}
    for mode in ("two_kernels", "path"):
        for chains in (1, 3):
            images[mode, chains] = render(r, mode, width, chains)
            assert r.launch_mode() == mode and r.node_width() == width
            assert np.array_equal(bits(images[mode, chains]), bits(want)), "%s, width %d, %d chains" % (mode, width, chains)
    first = images["two_kernels", 1]
    assert all(np.array_equal(bits(first), bits(img)) for img in images.values())
    owner = distributed.tile_owner(W, H, 3)
    mine = tuple(int(t) for t in range(3) if t % 3 == 1)
    part = render(r, "two_kernels", width, 1, partition=(1, 3))
    assert np.array_equal(bits(part), bits(oracle_render("deck", n, mine))) and part[owner == 1].any() and not part[owner != 1].any()


# ---- two levels --------------------------------------------------------------------------------------------------------------------
TWO_LEVEL_CARDS = 4 ** 7
TWO_LEVEL_COUNTS = (1, 2, 65, 513)
APART, STACKED = [(0, 0, 0), (5.0, 0, 0)], [(0, 0, 0), (2.0 ** -9, 0, 2.0 ** -15)]     # the second instance a quarter of a gap behind the first


@functools.lru_cache(maxsize=None)
def two_level_answers():
    desc = ss.instanced_deck_scene(TWO_LEVEL_CARDS, STACKED)
    return Answers(desc, ss.stack_rays(cards("deck", TWO_LEVEL_CARDS)[0], TWO_LEVEL_COUNTS[-1], RAY_SEED))


def check_two_level(scene, r, what):
    a = two_level_answers()
    bound = two_level_bound(scene)
    print("%s: top + mesh min_first_leaf_stack %d" % (what, bound))
    assert bound >= NEED_4
    a.check(scene, TWO_LEVEL_COUNTS, what)
    o = OracleRenderer(a.orc, W, H)
    o.set_depth(3)
    o.set_seed(7)
    o.step(LAUNCHES)
    assert np.array_equal(bits(render(r)), bits(o.read_hdr())), what


def test_two_level_deck_instanced_twice():
    scene = make_scene(two_level_answers().case.desc, levels="two_level")
    check_two_level(scene, glaze_amd.RayTraceRenderer.new(scene.instance, scene, W, H), "the deck instanced twice")


def test_two_level_instances_moved_on_top_of_each_other():
    """update_transforms: two decks side by side (a ray meets one of them) become one interleaved deck; the mesh's hierarchy stays, the
    top level is rebuilt, and the spill area has to serve both levels"""
    desc = ss.instanced_deck_scene(TWO_LEVEL_CARDS, APART)
    scene = make_scene(desc, levels="two_level")
    r = glaze_amd.RayTraceRenderer.new(scene.instance, scene, W, H)
    render(r)
    r.update_transforms(two_level_answers().case.desc.transforms)
    check_two_level(scene, r, "two decks moved on top of each other")


# ---- the post stage ----------------------------------------------------------------------------------------------------------------
def test_first_hit_planes_and_guide_chain_through_the_deck(instance):
    """k_first_hit and k_guide_trace (which uses the first-hit pass's spill slots): the first card is a mirror, the rest stand behind it,
    and a large mirror behind the last card sends every ray that passed them all back through all of them"""
    n = DECK_CARDS_4["sah"]
    desc = ss.mirror_deck_scene(n)
    orc = OracleScene(desc)
    scene = glaze_amd.RayTraceScene.from_desc(instance, desc)
    bound = min_first_leaf_stack(scene.debug_bvh()[0], 4)
    print("mirror deck of %d: min_first_leaf_stack %d" % (n, bound))
    assert bound >= NEED_4
    r = glaze_amd.RayTraceRenderer.new(instance, scene, W, H)
    # first-hit planes: depth and instance of the pixel centres' rays are the oracle's closest hits of those rays
    o, d = (x.reshape(-1, 3) for x in r.debug_camera_rays())
    t, tri, inst, u, v = orc.trace_closest(o, d, 1e-4)
    depth, instance_bits = r.read_aov("normal_depth")[..., 3].ravel(), r.read_aov("albedo_instance")[..., 3].ravel().view(np.uint32)
    assert np.array_equal(bits(depth), bits(t)) and np.array_equal(instance_bits, inst)
    assert (inst == 2).mean() > 0.3 and (inst == 0).mean() > 0.05 and (inst == 1).mean() > 0.05      # the back mirror, the first card, a card between
    # the guide chain's rays are the oracle's path through the mirrors, bit for bit (tests/test_gpu_guides.py)
    B = 3
    r.set_guide_mode("through_specular", B)
    assert launch_constants(1, 0)[1] == (0.5, 0.5)
    orc_ren = OracleRenderer(orc, W, H)
    orc_ren.set_seed(1)
    orc_ren.set_depth(16)
    so, sd, alive = (x.reshape(-1, x.shape[-1]) if x.ndim == 3 else x.ravel() for x in r.debug_guide_chain(0))
    assert alive.all() and np.array_equal(bits(so), bits(o)) and np.array_equal(bits(sd), bits(d))
    compared = np.ones(W * H, bool)
    followed = []
    for L in range(1, B + 1):
        orc_ren.step(1)
        state = orc_ren.read_state().reshape(-1, 24)
        wi, point = state[:, 16:19], state[:, 20:23]
        idx = np.flatnonzero(compared)
        t, tri, inst, u, v = orc.trace_closest(so[idx], sd[idx], 1e-4)
        on_mirror = np.isfinite(t) & (inst != 1)
        compared = np.zeros(W * H, bool)
        compared[idx[on_mirror]] = True
        followed.append(int(compared.sum()))
        so, sd, alive = (x.reshape(-1, x.shape[-1]) if x.ndim == 3 else x.ravel() for x in r.debug_guide_chain(L))
        assert alive[compared].all()
        differ = (bits(so[compared]) != bits(point[compared])).any(-1) | (bits(sd[compared]) != bits(wi[compared])).any(-1)
        assert not differ.any(), "segment %d: %d of %d rays differ from the oracle's path" % (L, differ.sum(), compared.sum())
    print("guide chain: rays followed at vertices 1 .. %d: %s" % (B, followed))
    assert followed[0] > W * H // 3                               # off the last card, back through the deck


# ---- live changes ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("builder", ["lbvh", "sah"])
def test_refit_moves_spread_cards_into_the_deck(builder):
    """update_vertices in refit mode: the cards start side by side in x and are moved into the stack.  The topology stays the spread
    scene's -- the same radix tree over the card numbers, so min_first_leaf_stack of the refitted arrays is what the deck's own build gives
    (21 at 4^7 cards, 4-wide; asserted below) -- while every box now overlaps every other."""
    n = DECK_CARDS_4[builder]
    z, u = cards("deck", n)
    scene = make_scene(ss.cards_scene(z, u, True, ss.spread_shift(n)), builder)
    r = glaze_amd.RayTraceRenderer.new(scene.instance, scene, W, H)
    before = scene.debug_bvh()[0][:, 12:16].copy()
    render(r)
    r.update_vertices(description("deck", n).vertices, 0, "refit")
    assert r.geometry_update_info().mode == glaze_amd.abi.GEOMETRY_REFIT
    nodes = scene.debug_bvh()[0]
    assert np.array_equal(nodes[:, 12:16], before)                 # the links did not move
    bound = min_first_leaf_stack(nodes, 4)
    print("refitted deck of %d, %s: min_first_leaf_stack %d" % (n, builder, bound))
    assert bound >= NEED_4
    a = answers("deck", n)
    a.check(scene, (2, 65, ray_counts(n)[-1]), "refitted deck, %s" % builder)
    fresh = make_scene(description("deck", n), builder)
    c = a.case
    for got, want in zip(scene.debug_trace_closest(c.o, c.d), fresh.debug_trace_closest(c.o, c.d)):
        assert np.array_equal(bits(got) if got.dtype == np.float32 else got, bits(want) if want.dtype == np.float32 else want)
    want = oracle_render("deck", n)
    for mode in ("two_kernels", "path"):
        assert np.array_equal(bits(render(r, mode)), bits(want)), mode
    assert np.array_equal(bits(render(glaze_amd.RayTraceRenderer.new(fresh.instance, fresh, W, H))), bits(want))


@pytest.mark.parametrize("mode", ["two_kernels", "path"])
def test_change_scene_from_the_cube_to_the_deck(instance, mode):
    """a live renderer sized for the cube (no spill to speak of) is handed the deck: its spill area has to follow the new scene's bound"""
    n = DECK_CARDS_4["sah"]
    r = glaze_amd.RayTraceRenderer.new(instance, glaze_amd.RayTraceScene.from_desc(instance, cube_scene()), W, H)
    render(r, mode)
    deck = glaze_amd.RayTraceScene.from_desc(instance, description("deck", n))
    assert min_first_leaf_stack(deck.debug_bvh()[0], 4) >= NEED_4
    r.change_scene(deck)
    assert np.array_equal(bits(render(r, mode)), bits(oracle_render("deck", n))), mode
