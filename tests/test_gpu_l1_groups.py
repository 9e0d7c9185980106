"""The unit-group pipeline of comap_l1_average: COMAP_GROUPS splits pass B,
the median and the tail into unit groups, COMAP_L1_PIPE=chain|alt chooses how the groups
are scheduled over the two streams.

No sum changes its order with the grouping (pass B is per tile, the median per series,
the sums and constants per (unit, band), the finish per tile), so at any group count and
either schedule every Level-2 output, needc and the pass fractions must equal the
one-group run's exactly -- NaN and +-inf positions included.  Both settings are read when
a plan is created, so every run builds a fresh GPUObservation.

Inputs (tests/golden/variants.py, the smallest that reach each branch): f3 = 6 units with
both scans >= 2w (groups of unequal size at 4); tinyscan = 3 units, two of them 3 and 4
samples long (bands the median skips, a group of skipped bands only, the count clamped
to the units); constel / calib = 1 unit (the clamp to one group); nan / infodd = the
special-row path, whose tail stays ungrouped.
"""
import os
import sys

import numpy as np
import pytest

from comapreduce_amd.pipeline.datahandling import COMAPLevel2, level1_from_dict

pytestmark = pytest.mark.gpu

KEYS = ('atmosphere/fit_values', 'averaged_tod/tod', 'averaged_tod/tod_original', 'averaged_tod/weights')
NAMES = ('f3', 'tinyscan', 'constel', 'calib', 'nan', 'infodd')
SETTINGS = [(g, pipe) for pipe in ('chain', 'alt') for g in (2, 3, 4)]

_gen = {}     # the last input made (one slot: f3 is 1.5 GB on the host)
_ref = {}     # name -> the one-group result, computed once and left unchanged


def _make(name):
    if name not in _gen:
        sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
        import variants
        _gen.clear()
        _gen[name] = variants.make(name)
    return _gen[name]


def _reduce(name):
    """The three stages on a fresh observation (a new plan): ({key: host array}, needc,
    pass fractions, pass-B launches of the averaging stage, units)."""
    from comapreduce_amd import Analysis as A
    data = level1_from_dict(_make(name))
    level2 = COMAPLevel2(filename='/nonexistent/none.hd5')
    stages = (A.MeasureSystemTemperature, A.AtmosphereRemoval, A.Level1AveragingGainCorrection)
    for cls in stages[:2]:
        st = cls(level2=level2)
        assert st(data, level2)
        level2.update(st)
    obs = data._gpu_observation
    obs.profile(2)
    obs.profile_collect()
    st = stages[2](level2=level2)
    assert st(data, level2)
    level2.update(st)
    launches = obs.profile_collect()['band_sums'][1]
    obs.profile(False)
    keys = KEYS + tuple(sorted(k for k in level2.keys() if k.startswith('vane/')))
    out = {k: np.array(level2[k]) for k in keys}
    res = (out, obs.debug(10), obs.pass_fractions(), launches, len(obs.units))
    obs.close()
    return res


def _one_group(name, monkeypatch):
    if name not in _ref:
        monkeypatch.setenv('COMAP_GROUPS', '1')
        monkeypatch.delenv('COMAP_L1_PIPE', raising=False)
        _ref[name] = _reduce(name)
        assert _ref[name][3] == 1
    return _ref[name]


def _assert_same(got, ref, what):
    out, need, frac = got[:3]
    rout, rneed, rfrac = ref[:3]
    assert sorted(out) == sorted(rout), what
    assert any(k.startswith('vane/') for k in out), what
    for k in out:
        assert out[k].shape == rout[k].shape and out[k].dtype == rout[k].dtype, (what, k)
        assert np.array_equal(out[k], rout[k], equal_nan=True), (what, k)
    assert np.array_equal(need, rneed), what
    assert frac == rfrac, (what, frac, rfrac)


@pytest.mark.parametrize('groups,pipe', SETTINGS)
@pytest.mark.parametrize('name', NAMES)
def test_groups_and_schedules_equal_one_group(name, groups, pipe, monkeypatch):
    ref = _one_group(name, monkeypatch)
    monkeypatch.setenv('COMAP_GROUPS', str(groups))
    monkeypatch.setenv('COMAP_L1_PIPE', pipe)
    got = _reduce(name)
    units = got[4]
    assert units == ref[4]
    assert got[3] == min(groups, units), (got[3], groups, units)     # the setting took effect; clamped to the units
    assert np.nanmax(np.abs(ref[0]['averaged_tod/tod'])) > 0
    _assert_same(got, ref, (name, groups, pipe))


def test_default_is_deterministic(monkeypatch):
    monkeypatch.delenv('COMAP_GROUPS', raising=False)
    monkeypatch.delenv('COMAP_L1_PIPE', raising=False)
    a = _reduce('f3')
    b = _reduce('f3')
    assert a[3] == b[3] >= 1
    _assert_same(a, b, 'f3 twice at the default')
    _assert_same(a, _one_group('f3', monkeypatch), 'f3 default against one group')


def test_unknown_schedule_is_refused(monkeypatch):
    from comapreduce_amd import _native as N
    from comapreduce_amd.gpu import GPUObservation
    monkeypatch.setenv('COMAP_L1_PIPE', 'sometimes')
    with pytest.raises(N.NativeError):
        GPUObservation(level1_from_dict(_make('constel')))
