"""The references of tests/test_gpu_stack_spill.py, checked without a GPU: the stack bounds on hand-made node arrays, the LDS level
counts the GPU cases assume against the headers, and the float64 brute force against the oracle on the deck and the comb -- with the
share of rays the brute force leaves out held under its cap for the very ray sets the GPU cases trace."""
import os
import re

import numpy as np
import pytest

from oracle.pyoracle import OracleScene

import stack_scenes as ss
import test_gpu_stack_spill as gpu_cases
from trace_ref import EMPTY_CHILD, MAX_DROPPED, RayCase, brute_force, first_leaf_stack_along_z, min_first_leaf_stack

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "glaze_amd", "csrc")


def test_lds_stack_levels_are_what_the_spill_cases_assume():
    """the two numbers live in kernels.h and device/tuning.h; the spill cases are sized for them"""
    kernels = open(os.path.join(CSRC, "kernels.h")).read()
    tuning = open(os.path.join(CSRC, "device", "tuning.h")).read()
    four = re.findall(r"^constexpr\s+int\s+kTraversalLdsStack\s*=\s*(\d+)\s*;", kernels, re.M)
    eight = re.findall(r"^#define\s+GLZ_TRACE8_STACK\s+(\d+)\s*$", tuning, re.M)
    assert four == [str(gpu_cases.LDS_LEVELS_4)] and eight == [str(gpu_cases.LDS_LEVELS_8)]
    assert (gpu_cases.LDS_LEVELS_4, gpu_cases.LDS_LEVELS_8, gpu_cases.MARGIN) == (17, 28, 4)


# ---- the bounds on hand-made node arrays ------------------------------------------------------------------------------------------
def nodes_of(children, width, z=None):
    """children: per node a list of links (>= 0 inner, < 0 leaf); z: per node a list of (lo, hi) quantised bounds along z"""
    out = np.zeros((len(children), 4 * width), np.uint32)
    links = np.full((len(children), width), EMPTY_CHILD, np.int64)
    for i, ch in enumerate(children):
        links[i, :len(ch)] = ch
        for k, (lo, hi) in enumerate(z[i] if z else []):
            out[i, 3 * k + 2] = lo | (hi << 16)
    out[:, 3 * width:] = links.astype(np.int32).view(np.uint32)
    return out


@pytest.mark.parametrize("width", [4, 8])
def test_min_first_leaf_stack_on_hand_made_trees(width):
    full = list(range(-1, -1 - width, -1))
    assert min_first_leaf_stack(nodes_of([full], width), width) == width - 1                         # one node of leaves
    assert min_first_leaf_stack(nodes_of([[-1, -2]], width), width) == 1                             # empty slots do not count
    assert min_first_leaf_stack(nodes_of([[-1]], width), width) == 0                                 # the scene of one leaf
    # two levels, every slot taken: (w - 1) a level
    two = [[1 + k for k in range(width)]] + [full] * width
    assert min_first_leaf_stack(nodes_of(two, width), width) == 2 * (width - 1)
    # the shallowest leaf decides: a leaf next to the root's inner children
    assert min_first_leaf_stack(nodes_of([[1, 2, -9], full, full], width), width) == 2
    # an unbalanced tree: root (3 children) -> node 1 (2 children) -> node 2 (full); the other leaves hang deeper than node 1's own leaf
    deep = [[1, 3, 4], [2, -1], full, full, full]
    assert min_first_leaf_stack(nodes_of(deep, width), width) == 2 + 1
    assert min_first_leaf_stack(nodes_of(deep, width), width, root=2) == width - 1
    # a chain: the root's own leaf is reached with one entry whatever the chain's length
    chain = [[k + 1, -(k + 1)] for k in range(30)] + [[-100, -101]]
    assert min_first_leaf_stack(nodes_of(chain, width), width) == 1
    with pytest.raises(ValueError):
        min_first_leaf_stack(nodes_of([[0, -1]], width), width)                                       # a node that links to itself
    with pytest.raises(ValueError):
        min_first_leaf_stack(np.zeros((1, 16), np.uint32), 8)


@pytest.mark.parametrize("width", [4, 8])
def test_first_leaf_stack_along_z_on_a_hand_made_chain(width):
    """a chain along z whose root holds the FARTHEST leaf: node k = (inner: the rest below, leaf at z = 100 - k)"""
    n = 20
    chain = [[k + 1, -(k + 1)] for k in range(n)] + [[-100, -101]]
    z = [[(0, 99 - k), (100 - k, 100 - k)] for k in range(n)] + [[(0, 0), (1, 1)]]
    nodes = nodes_of(chain, width, z)
    assert first_leaf_stack_along_z(nodes, width, +1, False) == n + 1          # +z, nearest first: down the whole chain before the first leaf
    assert first_leaf_stack_along_z(nodes, width, -1, True) == n + 1           # -z, farthest first: the same
    assert first_leaf_stack_along_z(nodes, width, -1, False) == 1              # -z, nearest first: the root's own leaf
    assert first_leaf_stack_along_z(nodes, width, +1, True) == 1
    # children that tie on the bound are all followed, and the smaller result stands
    z[0] = [(0, 99), (0, 100)]
    assert first_leaf_stack_along_z(nodes_of(chain, width, z), width, +1, False) == 1


# ---- the brute force --------------------------------------------------------------------------------------------------------------
def test_brute_force_on_single_triangles():
    tri = np.array([[[0, 0, 1], [1, 0, 1], [0, 1, 1]], [[0, 0, 1], [1, 0, 1], [0, 1, 1]], [[0, 0, 3], [1, 0, 3], [0, 1, 3]]], np.float64)
    o = np.array([[0.25, 0.25, 0], [0.25, 0.25, 4], [2, 2, 0], [0.5, 0.5 - 1e-6, 0], [0.25, 0.25, 0]], np.float32)
    d = np.array([[0, 0, 1], [0, 0, -1], [0, 0, 1], [0, 0, 1], [1, 0, 0]], np.float32)
    closest, near, far = brute_force(tri, o, d, [(1e-4, None), (1e-3, 0.5), (1e-3, np.full(5, 2.0, np.float32))])
    assert closest.tri.tolist() == [0, 2, -1, 0, -1] and np.allclose(closest.t[[0, 1, 3]], [1, 1, 1]) and np.isinf(closest.t[[2, 4]]).all()
    assert closest.keep.tolist() == [True, True, True, False, True]            # the fourth ray runs along the hypotenuse
    assert near.any.tolist() == [False] * 5 and far.any.tolist() == [True, True, False, True, False]
    assert far.keep_any.tolist() == [True, True, True, False, True]
    # a limit that falls on a triangle is nobody's to decide
    at = brute_force(tri, o[:1], d[:1], [(1e-3, np.float32(1.0))])[0]
    assert not at.keep_any[0]


FAMILIES = {"deck": 1024, "comb": gpu_cases.COMB_CARDS}


@pytest.mark.parametrize("paired", [True, False], ids=["paired", "unpaired"])
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_oracle_agrees_with_the_brute_force(family, paired):
    """the oracle (the float32 tracer every device result must equal bit for bit) against float64 on both families, at every ray count"""
    n = FAMILIES[family]
    z = gpu_cases.cards(family, n)[0]
    desc = ss.cards_scene(*gpu_cases.cards(family, n), paired=paired)
    case = RayCase(desc, ss.stack_rays(z, ss.RAY_COUNTS[-1], gpu_cases.RAY_SEED))
    orc = OracleScene(desc)
    t, tri, inst, _, _ = orc.trace_closest(case.o, case.d, 1e-4)
    hits = [orc.trace_any(case.o, case.d, tm) for tm in case.tmax]
    for count in ss.RAY_COUNTS:
        case.check_closest(t[:count], tri[:count], inst[:count], count)
        for which, hit in enumerate(hits):
            case.check_any(which, hit[:count], count)
    kinds = ss.kinds_of(case.n)
    hit = np.isfinite(t)
    assert not hit[np.char.startswith(kinds, "off")].any() and hit[np.char.startswith(kinds, "on")].all()
    if family == "deck":                                              # the band's rays pass some cards and hit one of the next
        first, last = tri[kinds == "band +z"] // 2, n - 1 - tri[kinds == "band -z"] // 2
        assert hit[np.char.startswith(kinds, "band")].all() and (first > 0).all() and (last > 0).all() and np.median(first) <= 3
    assert hits[0].mean() > hits[1].mean() + 0.01                                                       # the limit between two cards decides
    # coincident cards: the smaller world triangle wins
    twins = np.flatnonzero(z[1:] == z[:-1]) + 1
    assert twins.size and not np.isin(tri[hit] // 2, twins).any()


def test_the_ray_sets_of_the_gpu_cases_stay_under_the_drop_cap():
    """A condition on the chosen seeds: the brute force alone, on the ray sets of tests/test_gpu_stack_spill.py as they are, may leave
    out at most 1 % of any of them."""
    for family, n in [("deck", c) for c in sorted(set(gpu_cases.DECK_CARDS_4.values()))] + [("comb", gpu_cases.COMB_CARDS)]:
        counts = gpu_cases.ray_counts(n)
        case = RayCase(gpu_cases.description(family, n), ss.stack_rays(gpu_cases.cards(family, n)[0], counts[-1], gpu_cases.RAY_SEED))
        for count in counts:
            assert case.dropped(count) <= MAX_DROPPED, (family, n, count)
    desc = ss.instanced_deck_scene(gpu_cases.TWO_LEVEL_CARDS, gpu_cases.STACKED)
    case = RayCase(desc, ss.stack_rays(gpu_cases.cards("deck", gpu_cases.TWO_LEVEL_CARDS)[0], gpu_cases.TWO_LEVEL_COUNTS[-1], gpu_cases.RAY_SEED))
    for count in gpu_cases.TWO_LEVEL_COUNTS:
        assert case.dropped(count) <= MAX_DROPPED, ("two-level", count)
