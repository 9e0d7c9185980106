"""Split-map labels (destriper.split_labels) on hand-made feed / observation arrays, and the
.ini path: [Inputs] split_maps reaches run_destriper.main as a list of split kinds."""
import numpy as np
import pytest

from comapreduce_amd.mapmaking.destriper import split_labels

L = 4
#            offsets:  0      1      2      3      4      5
FEED = np.repeat([12, 3, 3, 12, 7, 3], L)
OBS = np.repeat([900, 900, 41, 41, 41, 900], L)


def test_label_order_and_names():
    lab, names = split_labels('feed', FEED, OBS, L)
    assert lab.dtype == np.int32 and lab.shape == (6,)
    assert names == ['Feed03', 'Feed07', 'Feed12']                 # sorted unique feeds, the reference's spelling
    assert lab.tolist() == [2, 0, 0, 2, 1, 0]
    lab, names = split_labels('obsid', FEED, OBS.astype(np.float64), L)
    assert names == ['Obs41', 'Obs900']
    assert lab.tolist() == [1, 1, 0, 0, 0, 1]


def test_values_fix_the_label_set():
    # a member no sample has (feed 5) is a label without offsets; labels index the given set
    lab, names = split_labels('feed', FEED, OBS, L, values=[12, 3, 5, 7, 3])
    assert names == ['Feed03', 'Feed05', 'Feed07', 'Feed12']
    assert lab.tolist() == [3, 0, 0, 3, 2, 0] and 1 not in lab
    # a sample whose feed is no member is left out of every split
    lab, names = split_labels('feed', FEED, OBS, L, values=[3, 12])
    assert names == ['Feed03', 'Feed12'] and lab.tolist() == [1, 0, 0, 1, -1, 0]
    lab, names = split_labels('obsid', FEED, OBS, L, values=[41, 900, 1000])
    assert names == ['Obs41', 'Obs900', 'Obs1000'] and lab.tolist() == [1, 1, 0, 0, 0, 1]


def test_label_changing_inside_an_offset_raises():
    feed = FEED.copy()
    feed[2 * L + 1] = 12
    with pytest.raises(ValueError, match='offset 2'):
        split_labels('feed', feed, OBS, L)
    split_labels('obsid', feed, OBS, L)                            # the observations are still whole
    with pytest.raises(ValueError, match='offset 2'):               # 900 900 | 900 41 ...: the first mixed offset
        split_labels('obsid', FEED, np.roll(OBS, 1), L)


def test_samples_must_be_whole_offsets():
    with pytest.raises(ValueError, match='multiple of offset_length'):
        split_labels('feed', FEED[:-1], OBS[:-1], L)
    with pytest.raises(ValueError):
        split_labels('scan', FEED, OBS, L)


INI = """[Inputs]
filelistname : filelist.txt
prefix : t
feeds : 1, 2
feed_weights : None
output_dir : maps/t
offset_length = 50
niter : 30
threshold : -6
nypix : 12
nxpix : 12
cdelt : -0.0166666,0.0166666
crpix : 6, 6
crval : 11:20:00,+52:00:00
ctype : RA---CAR, DEC--CAR
healpix : False
{extra}
[ReadData]
calibration : False
calibrator : TauA
use_gain_filter : True
"""


@pytest.mark.parametrize('line,want', [('split_maps : feed, obsid', ['feed', 'obsid']), ('split_maps : feed', ['feed']),
                                       ('', None), ('split_maps : None', None)])
def test_ini_hands_split_maps_to_main(tmp_path, monkeypatch, line, want):
    from comapreduce_amd.mapmaking import run_destriper as R
    got = {}
    monkeypatch.setattr(R, 'main', lambda *a, **kw: got.update(kw))
    path = tmp_path / 'p.ini'
    path.write_text(INI.format(extra=line))
    R.cli([str(path)])
    assert got['split'] == want and got['ground'] is False


def test_split_with_ground_raises_before_any_file_is_read():
    from comapreduce_amd.mapmaking import run_destriper as R
    with pytest.raises(NotImplementedError):
        R.main('/nonexistent/filelist.txt', ground=True, split=['feed'])
