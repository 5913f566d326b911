"""The size check of scene creation: the tracers address nodes, leaf records, instance records and spilt stack words with 32-bit byte
offsets, so a hierarchy one of whose tables would reach 2^32 bytes is refused with GLZ_E_INVALID_DATA and a message.

Such a scene cannot be built in a test (64 M leaf records are 4 GB), so the check is called with the counts alone, through
glz_host_traversal_offsets_fit -- the function Accel runs on what it has built; nothing is allocated, and no device is needed."""
import pytest

from glaze_amd import abi

E_INVALID_DATA = -3
# counts of a scene that fits: the 21 M triangle scene's order of magnitude, a full persistent grid (256 CUs x 8 blocks x 256 lanes), a deep tree
FITS = dict(n_nodes=7_000_000, n_nodes8=3_500_000, n_leaves=12_000_000, n_instances=1_000_000, grid_lanes=256 * 8 * 256, overflow_depth=120)
ORDER = ("n_nodes", "n_nodes8", "n_leaves", "n_instances", "grid_lanes", "overflow_depth")


def fit(**changed):
    return abi.lib().glz_host_traversal_offsets_fit(*[dict(FITS, **changed)[k] for k in ORDER])


def test_counts_of_a_large_scene_fit():
    assert fit() == 0
    assert fit(n_nodes=0, n_nodes8=0, n_leaves=0, n_instances=0, grid_lanes=0, overflow_depth=0) == 0


# first count at which the table's bytes reach 2^32, and what the message must name
LIMITS = [("n_nodes", 2**32 // 64, "4-wide nodes"), ("n_nodes8", 2**32 // 128, "8-wide nodes"), ("n_leaves", 2**32 // 64, "leaf records"),
          ("n_instances", -(-2**32 // 192), "instance records")]


@pytest.mark.parametrize("field,first_refused,named", LIMITS)
def test_a_table_of_2_to_the_32_bytes_is_refused(field, first_refused, named):
    assert fit(**{field: first_refused - 1}) == 0
    for n in (first_refused, first_refused + 1, 2**40, 2**64 - 1):
        assert fit(**{field: n}) == E_INVALID_DATA, n
        err = abi.last_error()
        assert err.status == E_INVALID_DATA and named in str(err) and "2^32" in str(err)


def test_a_spill_area_of_2_to_the_32_bytes_is_refused():
    lanes = FITS["grid_lanes"]                      # 2^19 lanes: 2^11 words each reach 2^30 words
    assert fit(overflow_depth=2**11 - 1) == 0
    for lanes_, depth in ((lanes, 2**11), (lanes, 2**11 + 1), (2**30, 1), (1, 2**30), (2**33, 2**33), (2**63, 2), (2**64 - 1, 2**64 - 1)):
        assert fit(grid_lanes=lanes_, overflow_depth=depth) == E_INVALID_DATA, (lanes_, depth)
        assert "spill" in str(abi.last_error())
    assert fit(grid_lanes=2**30 - 1, overflow_depth=1) == 0 and fit(grid_lanes=1, overflow_depth=2**30 - 1) == 0
