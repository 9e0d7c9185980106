"""merge_ground_tables: the ranks' ground-fit tables joined into the one a single rank holding
all samples would report, and the check that no (observation, feed) lives on two ranks.  Pure
NumPy on hand-made rank tables, no GPU."""
import numpy as np
import pytest

from comapreduce_amd.mapmaking.destriper import merge_ground_tables


def table(obsids, feeds, held, base):
    """A rank's table: slope = base + 10 i + j, level = -slope, wrapped where i + j is odd."""
    obsids, feeds, held = np.asarray(obsids), np.asarray(feeds), np.asarray(held, bool)
    i, j = np.meshgrid(np.arange(obsids.size), np.arange(feeds.size), indexing='ij')
    slope = np.where(held, base + 10.0 * i + j, 0.0)
    return {'obsids': obsids, 'feeds': feeds, 'slope': slope, 'level': -slope, 'wrapped': held & ((i + j) % 2 == 1),
            'held': held}


def test_union_grid_is_sorted_and_unheld_pairs_are_zero():
    # rank 0: observations 30 and 10 (sorted locally: 10, 30), feeds 1 and 5, (30, 5) absent;
    # rank 1: observation 20, feeds 5 and 12
    a = table([10, 30], [1, 5], [[1, 1], [1, 0]], 100.0)
    b = table([20], [5, 12], [[1, 1]], 200.0)
    m = merge_ground_tables([a, b])
    assert np.array_equal(m['obsids'], [10, 20, 30]) and np.array_equal(m['feeds'], [1, 5, 12])
    want = np.array([[100.0, 101.0, 0.0],
                     [0.0, 200.0, 201.0],
                     [110.0, 0.0, 0.0]])
    assert np.array_equal(m['slope'], want) and np.array_equal(m['level'], -want)
    assert m['wrapped'].dtype == bool
    assert np.array_equal(m['wrapped'], [[False, True, False], [False, False, True], [True, False, False]])
    # the order of the ranks does not matter
    m2 = merge_ground_tables([b, a])
    for k in m:
        assert np.array_equal(m[k], m2[k]), k


def test_one_rank_is_returned_unchanged():
    a = table([10, 30], [1, 5, 9], [[1, 1, 0], [1, 0, 1]], 3.0)
    m = merge_ground_tables([a])
    for k in ('obsids', 'feeds', 'slope', 'level', 'wrapped'):
        assert np.array_equal(m[k], a[k]), k


def test_feeds_that_differ_per_rank_inside_one_observation():
    # one observation split by feed: rank 0 feed 1, rank 1 feeds 5 and 12 of both observations
    a = table([10, 20], [1], [[1], [1]], 1.0)
    b = table([10, 20], [5, 12], [[1, 1], [0, 1]], 50.0)
    m = merge_ground_tables([a, b])
    assert m['slope'].shape == (2, 3)
    assert np.array_equal(m['slope'], [[1.0, 50.0, 51.0], [11.0, 0.0, 61.0]])


def test_pair_on_two_ranks_raises():
    a = table([10, 20], [1, 5], [[1, 1], [0, 0]], 1.0)
    b = table([10, 20], [5, 12], [[1, 0], [1, 1]], 7.0)           # (10, 5) again
    with pytest.raises(ValueError, match='observation 10, feed 5 .* ranks 0 and 1'):
        merge_ground_tables([a, b])
    # a pair both ranks list but only one holds is no duplicate
    b['held'][0, 0] = False
    m = merge_ground_tables([a, b])
    assert m['slope'][0, 1] == 2.0 and m['slope'][1, 1] == 17.0


def test_status_tables_without_a_fit_are_checked_too():
    """The set-up's exchange carries only the populated pairs (no slope yet)."""
    a = {'obsids': np.array([10]), 'feeds': np.array([1, 5]), 'held': np.array([[True, True]])}
    b = {'obsids': np.array([10]), 'feeds': np.array([5]), 'held': np.array([[True]])}
    with pytest.raises(ValueError, match='must live on one rank'):
        merge_ground_tables([a, b])
    m = merge_ground_tables([a, dict(b, obsids=np.array([11]))])
    assert m['slope'].shape == (2, 2) and not m['slope'].any()
