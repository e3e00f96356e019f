"""lhutil.stripe_counts (test infrastructure): the batch sizes tests/test_gpu_stripe_counts.py
sweeps per kernel.  The GPU test claims to meet every partial-wave and partial-workgroup residue
twice and a grid below, at and past 8 and 16 workgroups; these tests hold the generator to that,
so a GPU case never passes because its set lost a residue.  No GPU needed."""
import pytest

import lhutil

ORDER_EXTRA = (1023, 1024, 1025, 2047, 2048, 2049)


@pytest.mark.parametrize("tile", [1, 2, 3, 4, 9, 12, 32, 36, 128, 256, 1024])
def test_stripe_counts(tile):
    counts = lhutil.stripe_counts(tile)
    assert counts == sorted(set(counts)) and counts[0] == 1
    assert set(range(1, 2 * tile + 2)) <= set(counts)
    # every residue of the tile, and every number of whole tiles 0, 1, 2, at least twice over
    for r in range(tile):
        assert sum(1 for n in counts if n % tile == r) >= 2, r
    for g in (7, 8, 9, 15, 16, 17):
        assert {g * tile - 1, g * tile, g * tile + 1} <= set(counts), g
    assert counts[-1] == 17 * tile + 1
    # nothing else: the 1 .. 2T + 1 run and three sizes per grid
    assert set(counts) == set(range(1, 2 * tile + 2)) | {g * tile + d for g in lhutil.COUNT_GRIDS for d in (-1, 0, 1)}


def test_stripe_counts_known():
    assert lhutil.stripe_counts(1) == [1, 2, 3, 6, 7, 8, 9, 10, 14, 15, 16, 17, 18]
    assert lhutil.stripe_counts(4) == list(range(1, 10)) + [27, 28, 29, 31, 32, 33, 35, 36, 37, 59, 60, 61, 63, 64, 65,
                                                              67, 68, 69]
    assert len(lhutil.stripe_counts(256)) == 513 + 18 and lhutil.stripe_counts(256)[-1] == 4353
    assert lhutil.COUNT_GRIDS == (7, 8, 9, 15, 16, 17)


def test_stripe_counts_extra_and_grids():
    counts = lhutil.stripe_counts(1, extra=ORDER_EXTRA)
    assert counts[-6:] == list(ORDER_EXTRA) and counts[:-6] == lhutil.stripe_counts(1)
    assert lhutil.stripe_counts(1024, extra=ORDER_EXTRA)[:2049] == list(range(1, 2050))   # (already inside the run)
    short = lhutil.stripe_counts(12, grids=(7, 8, 9))
    assert short[-1] == 9 * 12 + 1 and set(range(1, 26)) <= set(short)
    assert lhutil.stripe_counts(3, extra=(5, 5, 100)) == sorted(set(lhutil.stripe_counts(3)) | {100})
    with pytest.raises(ValueError):
        lhutil.stripe_counts(0)
    with pytest.raises(ValueError):
        lhutil.stripe_counts(4, extra=(0,))


def test_a_wider_tile_covers_a_narrower_one():
    """The sweep gives a chain one case at its widest tile where that set holds the narrower
    kernels' sets whole (17 T' + 1 <= 2 T + 1): the bytewise apply's 128 over the scatter's 9,
    the order kernel's 1024 over the in-place apply's 1."""
    assert set(lhutil.stripe_counts(9)) <= set(lhutil.stripe_counts(128))
    assert set(lhutil.stripe_counts(1)) <= set(lhutil.stripe_counts(1024))
    assert not set(lhutil.stripe_counts(32)) <= set(lhutil.stripe_counts(256))
