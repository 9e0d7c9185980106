"""The regression formed from pass B's sums (default) against the per-channel path
(COMAP_L1_REGRESS=legacy: pass C + the per-channel solve for every (unit, band)),
on the same inputs, through the three stages.

Clean inputs: no pair may need pass C in the default mode, every pair takes it in
legacy mode, and the Level-2 outputs of the two agree to BOUND.  Inputs with NaN or
+-inf samples take the per-channel path in both modes (the special-row path needs every
channel's x), so there the two runs are the same code and must agree bit for bit.

BOUND: the largest fused-against-legacy relmax measured over the four clean cases is
recorded in DESIGN §3.1; the bound is 100 x that figure (room for other inputs' rounding)
and never looser than 1e-8, three orders inside the project's 1e-5.
"""
import os
import sys

import numpy as np
import pytest

from comapreduce_amd.pipeline.datahandling import COMAPLevel2, level1_from_dict

pytestmark = pytest.mark.gpu

MEASURED_RELMAX = 3.21e-13   # f3, averaged_tod/tod_original
BOUND = min(100 * MEASURED_RELMAX, 1e-8)
KEYS = ('averaged_tod/tod', 'averaged_tod/tod_original', 'averaged_tod/weights')


def relmax(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    fin = np.isfinite(b)
    assert np.array_equal(np.isfinite(a), fin), 'NaN pattern differs'
    return np.max(np.abs(a[fin] - b[fin])) / max(np.max(np.abs(b[fin])), 1e-300)


def _variants():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
    import variants
    return variants


def _reduce(gen):
    """The three stages on a fresh observation object (a new plan, which reads
    COMAP_L1_REGRESS when it is created): ({key: host array}, needc [U, 4], band on [U, 4])."""
    from comapreduce_amd import Analysis as A
    data = level1_from_dict(gen)
    level2 = COMAPLevel2(filename='/nonexistent/none.hd5')
    for cls in (A.MeasureSystemTemperature, A.AtmosphereRemoval, A.Level1AveragingGainCorrection):
        st = cls(level2=level2)
        assert st(data, level2)
        level2.update(st)
    obs = data._gpu_observation
    need = obs.debug(10).astype(int)
    band_on = obs.debug(9)[..., 1].astype(int)
    frac = obs.pass_fractions()
    out = {k: np.array(level2[k]) for k in KEYS}
    obs.close()
    return out, need, band_on, frac


def _both_modes(name, monkeypatch):
    gen = _variants().make(name)
    monkeypatch.delenv('COMAP_L1_REGRESS', raising=False)
    fused = _reduce(gen)
    monkeypatch.setenv('COMAP_L1_REGRESS', 'legacy')
    legacy = _reduce(gen)
    return fused, legacy


@pytest.mark.parametrize('name', ['f3', 'constel', 'calib', 'tinyscan'])
def test_fused_regression_matches_per_channel_path(name, monkeypatch):
    (out, need, band_on, frac), (ref, need_l, band_on_l, frac_l) = _both_modes(name, monkeypatch)
    assert band_on.any() and np.array_equal(band_on, band_on_l)
    assert not need.any(), need                 # no pair went through pass C
    assert need_l.all(), need_l                 # legacy: every pair did
    assert frac['regress'] == 0.0 and frac_l['regress'] > 0.0
    assert frac['band_sums'] == frac_l['band_sums']
    errs = {k: relmax(out[k], ref[k]) for k in KEYS}
    print(f'fused vs legacy {name}: ' + ' '.join(f'{k} {e:.3e}' for k, e in errs.items()))
    for k, e in errs.items():
        assert np.nanmax(np.abs(ref[k])) > 0, k
        assert e < BOUND, (name, k, e)


@pytest.mark.parametrize('name', ['nan', 'inf', 'infodd'])
def test_non_finite_inputs_take_per_channel_path(name, monkeypatch):
    (out, need, _, frac), (ref, need_l, _, frac_l) = _both_modes(name, monkeypatch)
    assert need.all(), need
    assert need_l.all(), need_l
    assert frac['regress'] == frac_l['regress'] > 0.0
    for k in KEYS:
        assert np.array_equal(out[k], ref[k], equal_nan=True), (name, k)     # NaN and +-inf positions included


def test_unknown_mode_is_refused(monkeypatch):
    from comapreduce_amd import _native as N
    from comapreduce_amd.gpu import GPUObservation
    monkeypatch.setenv('COMAP_L1_REGRESS', 'sometimes')
    with pytest.raises(N.NativeError):
        GPUObservation(level1_from_dict(_variants().make('constel')))
