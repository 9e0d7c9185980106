"""The noise prior's host side (no GPU): the stencil from a noise model, the red-noise fit's knee
frequency, the NumPy restatement of T v, the driver's parameter parsing, and the combinations that
are refused before any device call."""
import numpy as np
import pytest

from comapreduce_amd.mapmaking.destriper import (DeviceDestriper, fknee_from_red_noise, noise_prior_stencil,
                                                 prior_apply_reference, run_destriper, run_destriper_bands)
from comapreduce_amd.mapmaking.run_destriper import main, prior_params


def section(n, t):
    """The n-square finite section of the symmetric banded Toeplitz matrix with first row t."""
    row = np.zeros(n)
    m = min(n, t.size)
    row[:m] = t[:m]
    i = np.arange(n)
    return row[np.abs(i[:, None] - i[None, :])]


@pytest.mark.parametrize('taps', [1, 16, 64])
def test_stencil_sections_are_positive_definite(taps):
    t = noise_prior_stencil(0.2, -1.5, 50, taps=taps)
    assert t.shape == (taps + 1,) and np.all(np.isfinite(t)) and t[0] > 0
    assert t[0] == noise_prior_stencil(0.2, -1.5, 50, taps=1)[0]              # t[0] does not depend on the taps
    for n in (1, 5, 200):
        T = section(n, t)
        assert np.array_equal(T, T.T)
        lo = float(np.linalg.eigvalsh(T).min())
        print(f'taps {taps}, n {n}: smallest eigenvalue {lo:.4g} (t[0] = {t[0]:.4g})')
        assert lo > 0
    # the taper's price: a non-zero row sum (a weak zero-mean prior), a few per cent of t[0] at 16 taps
    if taps == 16:
        assert 0.03 < (t[0] + 2 * t[1:].sum()) / t[0] < 0.1


def test_stencil_matches_prior_apply_reference():
    t = noise_prior_stencil(0.2, -1.5, 50, taps=16)
    T = np.stack([prior_apply_reference(e, np.zeros(40, int), t[None]) for e in np.eye(40)], axis=1)
    assert np.array_equal(T, section(40, t))


def test_stencil_arguments():
    for bad in (dict(fknee=0.0), dict(fknee=np.nan), dict(alpha=0.0), dict(alpha=0.5), dict(taps=0), dict(taps=65)):
        kw = dict(fknee=0.2, alpha=-1.5, L=50)
        kw.update(bad)
        with pytest.raises(ValueError):
            noise_prior_stencil(**kw)


def test_fknee_from_red_noise():
    assert fknee_from_red_noise(1, 0.2 ** 0.75, -1.5) == pytest.approx(0.2, rel=1e-12)
    assert fknee_from_red_noise(2.0, 2.0, -1.0) == 1.0
    for sw, sr, a in ((0, 1, -1), (1, 0, -1), (-1, 1, -1), (1, -1, -1), (1, 1, 0), (1, 1, 1.5), (np.nan, 1, -1),
                      (1, np.inf, -1), (1, 1, np.nan)):
        assert np.isnan(fknee_from_red_noise(sw, sr, a)), (sw, sr, a)
    v = fknee_from_red_noise([1, 0, 1], [1, 1, 3], [-1, -1, -2])
    assert v[0] == 1.0 and np.isnan(v[1]) and v[2] == pytest.approx(3.0)


def test_prior_apply_reference():
    t = np.array([[2.0, -1.0], [3.0, 0.5]])
    gid = np.array([-1, 0, 0, 0, -1, 1, 1])
    v = np.array([9.0, 1.0, 2.0, 4.0, 9.0, 1.0, 10.0])
    want = [0.0, 2 * 1 - 2, 2 * 2 - 1 - 4, 2 * 4 - 2, 0.0, 3 * 1 + 5, 3 * 10 + 0.5]
    assert np.array_equal(prior_apply_reference(v, gid, t), want)
    assert not np.any(np.signbit(prior_apply_reference(-v, gid, t)[gid < 0]))
    with pytest.raises(ValueError, match='more than one run'):
        prior_apply_reference(v, np.array([0, 0, 1, 0, 1, 1, 1]), t)
    with pytest.raises(ValueError, match='out of range'):
        prior_apply_reference(v, np.array([0, 0, 0, 0, 1, 1, 2]), t)
    with pytest.raises(ValueError, match='out of range'):
        prior_apply_reference(v, np.array([0, 0, 0, 0, 1, 1, -2]), t)
    with pytest.raises(ValueError, match='K'):
        prior_apply_reference(v, gid, np.ones((2, 1)))
    with pytest.raises(ValueError, match='K'):
        prior_apply_reference(v, gid, np.ones((2, 66)))


def test_prior_params():
    assert prior_params({}) is None
    assert prior_params({'noise_prior': None}) is None and prior_params({'noise_prior': False}) is None
    assert prior_params({'noise_prior': 'fnoise'}) == 'fnoise'
    assert prior_params({'noise_prior': [0.2, -1.5]}) == (0.2, -1.5, 16)
    assert prior_params({'noise_prior': [0.2, -1.5, 32.0]}) == (0.2, -1.5, 32)
    for bad in ('fits', True, 0.2, [0.2], [0.2, -1.5, 16.0, 1.0], [0.2, 1.5], [-0.2, -1.5], [0.2, -1.5, 0.0],
                [0.2, -1.5, 65.0], [0.2, -1.5, 2.5], ['a', 'b']):
        with pytest.raises(ValueError):
            prior_params({'noise_prior': bad})


def test_refused_before_any_device_call():
    """prior with ground, with a 2-D tod, and through run_destriper_bands: NotImplementedError from
    the argument checks alone (no GPU here)."""
    n, L = 40, 10
    pix, tod, w = np.zeros(n, np.int32), np.zeros(n), np.ones(n)
    pair = (np.zeros(n // L, np.int32), np.ones((1, 2)))
    feed, obs = np.ones(n), np.ones(n)
    with pytest.raises(NotImplementedError, match='ground'):
        DeviceDestriper(pix, tod, w, L, 4, prior=pair, ground=(np.zeros(n), feed, obs))
    with pytest.raises(NotImplementedError, match='one band'):
        DeviceDestriper(pix, np.zeros((2, n)), np.ones((2, n)), L, 4, prior=pair)
    with pytest.raises(NotImplementedError, match='ground'):
        run_destriper(pix, tod, w, L, np.arange(4), az=np.zeros(n), feedid=feed, obsids=obs, ground=True, prior=pair)
    with pytest.raises(NotImplementedError, match='one band'):
        run_destriper(pix, np.zeros((2, n)), np.ones((2, n)), L, np.arange(4), prior=pair)
    with pytest.raises(NotImplementedError, match='one band'):
        run_destriper_bands(pix, np.zeros((2, n)), np.ones((2, n)), L, np.arange(4), prior=pair)
    with pytest.raises(ValueError, match='feedid'):
        run_destriper(pix, tod, w, L, np.arange(4), prior={'fknee': 0.2, 'alpha': -1.5})
    with pytest.raises(ValueError):
        DeviceDestriper(pix, tod, w, L, 4, prior=(pair[0],))
    with pytest.raises(NotImplementedError, match='ground_template'):
        main([], noise_prior=(0.2, -1.5), ground=True)
    with pytest.raises(ValueError):
        main([], noise_prior='fits')
