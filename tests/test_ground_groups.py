"""ground_groups: the (observation, feed) group of every destriper offset, in the
reference's order (op_Ax_with_ground, Destriper.py:279-287).  Pure NumPy, no GPU."""
import numpy as np
import pytest

from comapreduce_amd.mapmaking.destriper import ground_groups

L = 10


def _samples():
    """2 observations x 3 feeds with (obs 20, feed 5) absent; 2 offsets per present group,
    the groups deliberately not in sorted order."""
    combos = [(20, 1), (10, 5), (10, 1), (20, 12), (10, 12)]
    obs = np.concatenate([np.full(2 * L, o) for o, _ in combos])
    feed = np.concatenate([np.full(2 * L, f) for _, f in combos])
    return combos, feed, obs


def test_group_ids_follow_obs_major_feed_minor():
    combos, feed, obs = _samples()
    gid, uobs, ufeed = ground_groups(feed, obs, L)
    assert gid.dtype == np.int32 and gid.shape == (feed.size // L,)
    assert np.array_equal(uobs, [10, 20]) and np.array_equal(ufeed, [1, 5, 12])
    want = []
    for o, f in combos:
        i, j = int(np.searchsorted(uobs, o)), int(np.searchsorted(ufeed, f))
        want += [i * ufeed.size + j] * 2
    assert np.array_equal(gid, want)
    # the absent combination (obs 20, feed 5) is group 1 * 3 + 1, which no offset belongs to
    assert 4 not in gid and set(gid) == {0, 1, 2, 3, 5}


def test_offset_straddling_two_groups_raises():
    _, feed, obs = _samples()
    feed = feed.copy()
    feed[2 * L - 1] = 5          # the last sample of (20, 1)'s second offset moves to feed 5
    with pytest.raises(ValueError, match='straddles'):
        ground_groups(feed, obs, L)
    obs2 = obs.copy()
    obs2[5] = 10                 # an observation change inside an offset
    with pytest.raises(ValueError, match='straddles'):
        ground_groups(_samples()[1], obs2, L)


def test_length_mismatch_raises():
    _, feed, obs = _samples()
    with pytest.raises(ValueError):
        ground_groups(feed[:-L], obs, L)
    with pytest.raises(ValueError):
        ground_groups(feed[:-1], obs[:-1], L)      # not a multiple of the offset length


@pytest.mark.parametrize('line,want', [('', False), ('ground_template : True\n', True),
                                       ('ground_template : False\n', False)])
def test_ini_key_selects_the_ground_fit(golden_dir, tmp_path, monkeypatch, line, want):
    """[Inputs] ground_template reaches main(ground=...); absent means False."""
    import os
    from comapreduce_amd.mapmaking import run_destriper as rd
    src = open(os.path.join(golden_dir, 'params_case.ini')).read()
    assert '[Inputs]' in src and 'ground_template' not in src
    ini = tmp_path / 'p.ini'
    ini.write_text(src.replace('[Inputs]\n', '[Inputs]\n' + line, 1))
    seen = {}
    monkeypatch.setattr(rd, 'main', lambda *a, **kw: seen.update(kw))
    rd.cli([str(ini)])
    assert seen['ground'] is want
