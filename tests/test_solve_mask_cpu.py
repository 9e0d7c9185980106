"""The solve mask's host pieces (no GPU): ``mask_from_map`` on a hand-made 8 x 8 map, the mask's
validation, the .ini spellings of [Inputs] solve_mask, the FITS mask reader and ``write_map``'s extra
HDU, and the combinations that are refused before any device call."""
import numpy as np
import pytest

from comapreduce_amd.mapmaking.destriper import (DeviceDestriper, mask_from_map, run_destriper, run_destriper_bands,
                                                 solve_mask_flags)
from comapreduce_amd.mapmaking.fits import read_image_hdus, write_image_hdus
from comapreduce_amd.mapmaking.run_destriper import main, mask_params, read_solve_mask, write_map
from comapreduce_amd.tools.parser import Parser


def hand_made():
    """8 x 8, unit background of weight 4 (sigma 0.5): median 1; (3, 4) stands 3.0 above it (6 sigma),
    (6, 1) stands 2.0 below (4 sigma), (0, 0) is far off but unhit, (7, 7) stands 2.6 above (5.2
    sigma) in a corner, (5, 5) stands 1.0 above at weight 36 (6 sigma through its weight alone)."""
    m, w = np.ones((8, 8)), np.full((8, 8), 4.0)
    m[3, 4], m[6, 1], m[0, 0], m[7, 7], m[5, 5] = 4.0, -1.0, 99.0, 3.6, 2.0
    w[0, 0], w[5, 5] = 0.0, 36.0
    return m, w


def test_mask_from_map_by_hand():
    m, w = hand_made()
    seed = np.zeros((8, 8), bool)
    seed[3, 4] = seed[7, 7] = seed[5, 5] = True
    assert np.array_equal(mask_from_map(m, w, 5, 0), seed)
    once = seed.copy()
    for y, x in ((3, 4), (7, 7), (5, 5)):
        for dy, dx in ((1, 0), (-1, 0), (0, 1), (0, -1)):
            if 0 <= y + dy < 8 and 0 <= x + dx < 8:                     # the 3 x 3 cross, no wrap at the border
                once[y + dy, x + dx] = True
    assert np.array_equal(mask_from_map(m, w, 5, 1), once) and np.array_equal(mask_from_map(m, w, 5), once)
    assert once.sum() == 3 + 4 + 2 + 4 and not once[0, 7] and not once[7, 0]
    twice = mask_from_map(m, w, 5, 2)
    assert twice[3, 2] and twice[2, 3] and not twice[1, 2] and twice.sum() > once.sum()
    # the threshold is strict and two-sided: 4 sigma below passes at 5, is caught at 3.9
    assert not mask_from_map(m, w, 5, 0)[6, 1] and mask_from_map(m, w, 3.9, 0)[6, 1]
    assert not mask_from_map(m, w, 6.0, 0)[3, 4]                        # exactly 6 sigma is not > 6
    # an unhit pixel is never flagged and does not enter the median
    assert not mask_from_map(m, w, 0.1, 0)[0, 0]
    assert not mask_from_map(m, np.zeros((8, 8)), 5, 1).any()
    nan = m.copy()
    nan[2, 2] = np.nan                                                  # (unhit: it never enters)
    w2 = w.copy()
    w2[2, 2] = 0.0
    assert np.array_equal(mask_from_map(nan, w2, 5, 0), seed)
    for bad in ((m.reshape(-1), w.reshape(-1), 5, 1), (m, w[:4], 5, 1), (m, w, 0, 1), (m, w, np.nan, 1), (m, w, 5, -1)):
        with pytest.raises(ValueError):
            mask_from_map(*bad)


def test_solve_mask_flags():
    f = solve_mask_flags(np.array([0, 2, 0, -1]), 4)
    assert f.dtype == np.uint8 and f.tolist() == [0, 1, 0, 1]
    assert solve_mask_flags(np.array([[True, False], [False, True]]), 4, (2, 2)).tolist() == [1, 0, 0, 1]
    assert solve_mask_flags(np.array([0.0, 0.5]), 2).tolist() == [0, 1]
    for bad, npix, shape in ((np.zeros(3), 4, None), (np.zeros((2, 2)), 4, None), (np.zeros((2, 2)), 4, (1, 4)),
                             (np.zeros((1, 2, 2)), 4, None), (np.array([0.0, np.nan]), 2, None),
                             (np.array([0.0, np.inf]), 2, None), (np.array(['a', 'b']), 2, None)):
        with pytest.raises(ValueError, match='solve mask'):
            solve_mask_flags(bad, npix, shape)


def test_ini_spellings(tmp_path):
    assert mask_params({}) is None
    assert mask_params({'solve_mask': None}) is None and mask_params({'solve_mask': False}) is None
    assert mask_params({'solve_mask': 'masks/taua.fits'}) == 'masks/taua.fits'
    assert mask_params({'solve_mask': ['snr', 5.0]}) == ('snr', 5.0, 1)
    assert mask_params({'solve_mask': ['snr', 4.5, 2.0]}) == ('snr', 4.5, 2)
    assert mask_params({'solve_mask': ('snr', 5, 0)}) == ('snr', 5.0, 0)
    for bad in (True, 5.0, 'snr', ['snr'], ['snr', 0.0], ['snr', -1.0], ['snr', 'x'], ['snr', 5.0, 1.5],
                ['snr', 5.0, -1.0], ['snr', 5.0, 1.0, 2.0], ['a.fits', 'b.fits'], ['sigma', 5.0]):
        with pytest.raises(ValueError, match='solve_mask'):
            mask_params({'solve_mask': bad})
    ini = tmp_path / 'p.ini'
    ini.write_text('[Inputs]\nsolve_mask : snr, 5, 2   # two passes\n[Other]\nsolve_mask = maps/mask.fits\n'
                   '[Off]\nsolve_mask : None\n')
    p = Parser(str(ini))
    assert mask_params(p['Inputs']) == ('snr', 5.0, 2)
    assert mask_params(p['Other']) == 'maps/mask.fits'
    assert mask_params(p['Off']) is None


def test_fits_mask_and_the_extra_hdu(tmp_path):
    mask = np.zeros((6, 9))
    mask[2, 3] = 1.0
    mask[4, 8] = -2.5                                                   # non-zero means masked
    write_image_hdus(str(tmp_path / 'm.fits'), [(None, mask), ('Other', np.ones((6, 9)))])
    got = read_solve_mask(str(tmp_path / 'm.fits'), 6, 9)
    assert got.dtype == bool and got.shape == (6, 9) and np.array_equal(got, mask != 0)
    with pytest.raises(ValueError, match='solve_mask'):
        read_solve_mask(str(tmp_path / 'm.fits'), 9, 6)
    mask[0, 0] = np.nan
    write_image_hdus(str(tmp_path / 'nan.fits'), [(None, mask)])
    with pytest.raises(ValueError, match='NaN'):
        read_solve_mask(str(tmp_path / 'nan.fits'), 6, 9)

    # write_map: without a mask the file is the same bytes as before; with one, one more HDU
    class Cards:
        def to_header(self):
            return [('CRVAL1', 170.0)]

    rng = np.random.default_rng(0)
    maps = {'All': {'map': rng.standard_normal(54), 'naive': rng.standard_normal(54), 'weight': rng.random(54),
                    'hits': rng.integers(0, 5, 54).astype(float)}}
    info = {'wcs': Cards(), 'nxpix': 9, 'nypix': 6}
    write_map('t', maps, info, str(tmp_path / 'a'), 0)
    write_map('t', maps, info, str(tmp_path / 'b'), 0, solve_mask=None)
    write_map('t', maps, info, str(tmp_path / 'c'), 0, solve_mask=got.reshape(-1))
    a, b, c = (open(tmp_path / d / 'All_t_Band00.fits', 'rb').read() for d in 'abc')
    assert a == b and c[:len(a)] == a and len(c) > len(a)
    hdus = read_image_hdus(str(tmp_path / 'c' / 'All_t_Band00.fits'))
    assert [h.get('EXTNAME') for h, _ in hdus] == [None, 'Naive', 'Noise', 'Hits', 'SolveMask']
    assert np.array_equal(hdus[-1][1], got.astype(float)) and hdus[-1][0]['CRVAL1'] == 170.0


def test_refused_before_any_device_call():
    """ground, residual_cut, HEALPix and the per-band 'snr' form through the batched driver:
    NotImplementedError from the argument checks alone (no GPU here)."""
    n, L = 40, 10
    pix, tod, w = np.zeros(n, np.int32), np.zeros(n), np.ones(n)
    mask = np.zeros(4, bool)
    z = np.zeros(n)
    with pytest.raises(NotImplementedError, match='ground'):
        DeviceDestriper(pix, tod, w, L, 4, solve_mask=mask, ground=(z, z, z))
    with pytest.raises(NotImplementedError, match='residual_cut'):
        DeviceDestriper(pix, tod, w, L, 4, solve_mask=mask, residual_groups=(z, z), residual_cut=3.0)
    edges = np.arange(4)
    with pytest.raises(NotImplementedError, match='ground'):
        run_destriper(pix, tod, w, L, edges, az=z, feedid=z, obsids=z, ground=True, solve_mask=mask)
    with pytest.raises(NotImplementedError, match='HEALPix'):
        run_destriper(pix, tod, w, L, edges, healpix=True, solve_mask=mask)
    with pytest.raises(NotImplementedError, match='residual_cut'):
        run_destriper_bands(pix, np.stack([tod, tod]), np.stack([w, w]), L, edges, feedid=z, obsids=z, residual_cut=2.0,
                            solve_mask=mask)
    with pytest.raises(NotImplementedError, match='per band'):
        run_destriper_bands(pix, np.stack([tod, tod]), np.stack([w, w]), L, edges, solve_mask=('snr', 5))
    with pytest.raises(ValueError, match='map_shape'):
        run_destriper(pix, tod, w, L, edges, solve_mask=('snr', 5))
    for kw in (dict(ground=True), dict(residual_cut=2.0), dict(healpix=True)):
        with pytest.raises(NotImplementedError):
            main(['none.hd5'], solve_mask='mask.fits', **kw)
    with pytest.raises(ValueError, match='solve_mask'):
        main(['none.hd5'], solve_mask=['snr'])
