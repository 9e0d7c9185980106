"""The data prep's gather and cut kernels (csrc/prep_kernels.hip) call by call:
comap_prep_gather and comap_prep_cut through the C entry points on hand-built tables,
against plain NumPy restatements of the reference (get_tod / read_pixels,
COMAPData.py:300-376, 404-425; the NaN and empty-offset cuts, :550-568) and, for the
pixel ids, against astropy 4.3.1 / wcslib (tests/golden/golden_astro.npz).

The Sun-centric distance and colatitude are trigonometric leaves: the device's libm sits
an ulp or two from NumPy's, so where generic pointing goes through them (the Sun-cut
boundary and the finite samples of the non-finite test) they are held to the project's
bound for these leaves, 1e-12 max(max|ref|, 1) (test_comapdata.TRIG).  The scan-table and
cut tests compare every column with array_equal instead: the rows feeding the Sun
columns point at dec = +-90, ra = 0 under the rotation diag(1, -1, -1), where every
libm call is at a special value (sin 0, cos 0, acos +-1, asin 0, asin 1, atan2(0, x > 0)),
so the distance is exactly 180 (kept) or 0 (cut) and the colatitude pi or 0 on both sides.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from comapreduce_amd.mapmaking import astro
from comapreduce_amd.mapmaking.wcs import CelestialWCS, transform_to_1d

from test_astro_golden import MAPS, _points_near_cut, native_x

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
COLS = ('tod', 'w', 'az', 'el', 'ra', 'dec', 'feedid', 'obsid', 'pix')
F8_SENTINEL, INT_SENTINEL = 7.25, 77
# prep_kernels.hip: "a file of up to kScanLds scans keeps its table in LDS, a longer one
# is binary-searched in global memory" (constexpr int kScanLds = 128)
K_SCAN_LDS = 128
# the rotation under which dec = +-90, ra = 0 give exact Sun columns (module docstring)
EXACT_ROT = np.diag([1.0, -1.0, -1.0])
# a 1-degree all-sky CAR map: both poles and every (ra, dec) in (-180, 180) x [-90, 90] on it
WORLD = dict(crval=[0.0, 0.0], cdelt=[-1.0, 1.0], crpix=[181, 91], ctype=['RA---CAR', 'DEC--CAR'], nx=361, ny=181)


# ---------------------------------------------------------------- device calls
def _ctx():
    import torch
    from comapreduce_amd import _native as N
    dev = torch.device('cuda', 0)
    c = N.ctx(0)
    N.bind_stream(c, dev)
    return torch, N, dev, c


def _fresh(torch, N, dev, shape, dtype):
    """An output buffer: N.device_empty (NaN / -1 under COMAP_POISON=1), otherwise filled with a
    sentinel that no test input holds, so an element the kernel did not write shows."""
    t = N.device_empty(shape, dtype, dev)
    if not N.POISON:
        t.fill_(F8_SENTINEL if t.is_floating_point() else INT_SENTINEL)
    return t


def _untouched(a):
    from comapreduce_amd import _native as N
    if N.POISON:
        return bool(np.all(np.isnan(a)) if a.dtype.kind == 'f' else np.all(a == (255 if a.dtype == np.uint8 else -1)))
    return bool(np.all(a == (F8_SENTINEL if a.dtype.kind == 'f' else INT_SENTINEL)))


def scan_table(edges, L):
    """(first file sample, N = (end - start) // L * L, first output column) per scan."""
    edges = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    n = (edges[:, 1] - edges[:, 0]) // L * L
    col = np.concatenate(([0], np.cumsum(n)[:-1])).astype(np.int64)
    return np.stack([edges[:, 0], n, col], axis=1).astype(np.int64)


def map_wcs(m):
    from comapreduce_amd.mapmaking.prep import wcs_struct
    w = CelestialWCS(m['crval'], m['cdelt'], m['crpix'], m['ctype'])
    return w, wcs_struct({'wcs': w, 'nxpix': m['nx'], 'nypix': m['ny']})


def gather(t, wcs=None, pixels=None, offset=5, pad=3, **override):
    """One comap_prep_gather call on the tables of ``t``.  Returns (rc, message, columns as
    NumPy: tod / w [nb, rows, datasize], the others [rows, datasize]); the outputs are longer
    than the file's block by ``offset`` in front and ``pad`` behind (band stride included),
    and those margins must come back untouched."""
    torch, N, dev, c = _ctx()
    from comapreduce_amd.mapmaking.prep import PrepFile, PrepOut
    up = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a, dtype=dt), device=dev)  # noqa: E731
    scans = scan_table(t['edges'], t['L'])
    nrow, nb, ds = len(t['row_src']), len(t['bands']), int(scans[:, 1].sum())
    n = offset + nrow * ds + pad
    # (every device operand is bound to a name until the call has run)
    tod, az, el, ra, dec = (up(t[k], np.float64) for k in ('tod', 'az', 'el', 'ra', 'dec'))
    spike = None if t.get('spike') is None else up(t['spike'], np.uint8)
    dsc, drs, dps = up(scans, np.int64), up(t['row_src'], np.int32), up(t['pix_src'], np.int32)
    drf, drc, drw, drp = (up(t[k], dt) for k, dt in (('row_feed', np.int64), ('row_cal', np.float64),
                                                      ('row_w', np.float64), ('row_pct', np.float64)))
    dpx = None if pixels is None else up(pixels, np.int64)
    f8 = torch.float64
    o = {k: _fresh(torch, N, dev, (nb, n) if k in ('tod', 'w') else n,
                   torch.int64 if k in ('feedid', 'obsid') else torch.int32 if k == 'pix' else f8) for k in COLS}
    F, B, T = t['tod'].shape
    ss = (0, 0) if spike is None else (spike.shape[1] * spike.shape[2], spike.shape[2])
    pf = PrepFile(N.dptr(tod), B * T, T, N.dptr(az), N.dptr(el), N.dptr(ra), N.dptr(dec), T,
                  None if spike is None else N.dptr(spike), ss[0], ss[1], nrow, int(scans.shape[0]), ds,
                  N.dptr(dsc), N.dptr(drs), N.dptr(dps), N.dptr(drf), N.dptr(drc), N.dptr(drw), N.dptr(drp),
                  (ctypes.c_int32 * 4)(*(list(t['bands']) + [0] * 4)[:4]), nb,
                  (ctypes.c_double * 9)(*np.asarray(t['sun_rot'], dtype=np.float64).ravel()), int(t['obsid']),
                  None if dpx is None else N.dptr(dpx))
    for k, v in override.items():
        setattr(pf, k, v)
    d = N.dptr
    po = PrepOut(d(o['tod']), d(o['w']), n, d(o['az']), d(o['el']), d(o['ra']), d(o['dec']), d(o['feedid']),
                 d(o['obsid']), d(o['pix']), offset)
    rc = N.lib().comap_prep_gather(c, ctypes.byref(pf), None if wcs is None else ctypes.byref(wcs), ctypes.byref(po))
    torch.cuda.synchronize(dev)
    msg = N.lib().comap_last_error(c).decode() if rc else ''
    res = {}
    for k in COLS:
        a = o[k].cpu().numpy().reshape(-1, n)
        if rc == 0 and not override:
            assert _untouched(a[:, :offset]) and _untouched(a[:, n - pad:]), k
        res[k] = a if (rc or override) else a[:, offset:n - pad].reshape((nb, nrow, ds) if k in ('tod', 'w')
                                                                          else (nrow, ds))
    return rc, msg, res


# ---------------------------------------------------------------- the reference, restated
def with_matrix(mat):
    r = astro.Rotator()
    r.mat = np.asarray(mat, dtype=np.float64)
    return r


def reference_file(t, pixel_of=None, pixels=None):
    """get_tod (per band) and read_pixels of one file (COMAPData.py:300-376, 404-425) on the
    tables of ``t``: tod / cal, the spike, Sun, percentile and 10 % scan-edge cuts, bad rows
    left zero, the pixel row of output row i taken from file row pix_src[i].  The weights
    (1 / auto_rms^2), the percentiles and the Sun's rotation come from the tables; the
    high-pass is another kernel's."""
    edges, L = np.asarray(t['edges']).reshape(-1, 2), t['L']
    Ns = [int((end - start) // L * L) for start, end in edges]
    nrow, nb, ds = len(t['row_src']), len(t['bands']), sum(Ns)
    out = {k: np.zeros((nb, nrow, ds) if k in ('tod', 'w') else (nrow, ds)) for k in COLS}
    out['obsid'][:] = t['obsid']
    if pixels is not None:
        out['pix'][:] = pixels
    else:
        last = 0
        for (start, end), N in zip(edges, Ns):
            for row, ps in enumerate(t['pix_src']):
                if ps >= 0:
                    out['pix'][row, last:last + N] = pixel_of(t['ra'][ps, start:start + N],
                                                              t['dec'][ps, start:start + N])
            last += N
    rot = with_matrix(t['sun_rot'])
    with np.errstate(invalid='ignore'):
        for k, band in enumerate(t['bands']):
            for row, rs in enumerate(t['row_src']):
                if rs < 0:
                    continue
                tod_file = t['tod'][rs, band, :] / t['row_cal'][row, k]
                weights_file = np.ones(tod_file.size) * t['row_w'][row, k]
                az_file, el_file = t['az'][rs], t['el'][rs]
                ra, dec = t['ra'][rs], t['dec'][rs]
                theta, phi = (np.pi / 2. - dec * np.pi / 180.), ra * np.pi / 180.
                good = np.isfinite(ra) & np.isfinite(dec)
                theta[good], phi[good] = rot(theta[good], phi[good])
                ra_file = astro.haversine(0, 0, phi, theta) * 180.0 / np.pi
                dec_file = theta
                out['feedid'][row] = t['row_feed'][row]
                if t.get('spike') is not None:
                    weights_file[t['spike'][rs, band, :tod_file.size].astype(bool)] = 0
                weights_file[ra_file < 10] = 0
                az10, az90, el10, el90 = t['row_pct'][row]
                weights_file[(az_file < az10) | (az_file > az90)] = 0
                weights_file[(el_file < el10) | (el_file > el90)] = 0
                last = 0
                for (start, end), N in zip(edges, Ns):
                    Nten = int(N * 0.1)
                    weights_file[start:start + Nten] = 0
                    weights_file[start + N - Nten:start + N] = 0
                    out['tod'][k, row, last:last + N] = tod_file[start:start + N]
                    out['w'][k, row, last:last + N] = weights_file[start:start + N]
                    out['az'][row, last:last + N] = az_file[start:start + N]
                    out['el'][row, last:last + N] = el_file[start:start + N]
                    out['ra'][row, last:last + N] = ra_file[start:start + N]
                    out['dec'][row, last:last + N] = dec_file[start:start + N]
                    last += N
    for k in ('feedid', 'obsid'):
        out[k] = out[k].astype(np.int64)
    out['pix'] = out['pix'].astype(np.int64).astype(np.int32)
    return out


def assert_columns_equal(got, want, what):
    for k in COLS:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, (what, k)
        assert np.array_equal(got[k], want[k], equal_nan=(k not in ('feedid', 'obsid', 'pix'))), \
            (what, k, int(np.sum(got[k] != want[k])))


def one_row(ra, dec, chunk=None, sun_rot=None):
    """Tables for one output row holding ra / dec: one scan, or scans of ``chunk`` < 10 samples
    (L = 1, so int(N * 0.1) = 0: no scan-edge cut); unit weights, percentiles at -+inf."""
    T = int(ra.size)
    edges = [[0, T]] if chunk is None else [[a, min(a + chunk, T)] for a in range(0, T, chunk)]
    return dict(tod=np.ones((1, 1, T)), az=np.zeros((1, T)), el=np.zeros((1, T)), ra=ra[None].copy(),
                dec=dec[None].copy(), spike=None, edges=edges, L=1, row_src=[0], pix_src=[0], row_feed=[7],
                row_cal=np.ones((1, 4)), row_w=np.ones((1, 4)), row_pct=[[-np.inf, np.inf, -np.inf, np.inf]],
                bands=(0,), sun_rot=np.identity(3) if sun_rot is None else sun_rot, obsid=12345)


@pytest.fixture(scope='module')
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, 'golden_astro.npz'))


def golden_points(golden, name):
    """(lon, lat, astropy px, py) of a map: the scattered points, plus the central-row points
    of the zenithal maps."""
    keys = [f'wcs_{name}'] + ([f'wcs_{name}_row'] if name in ('sin', 'tan') else [])
    return tuple(np.concatenate([golden[f'{k}_{c}'] for k in keys]) for c in ('lon', 'lat', 'px', 'py'))


# ---------------------------------------------------------------- (a) device WCS vs astropy
@pytest.mark.parametrize('name,crval,cdelt,crpix,ctype,nx,ny,tol', MAPS, ids=[m[0] for m in MAPS])
def test_device_wcs_vs_wcslib(golden, name, crval, cdelt, crpix, ctype, nx, ny, tol):
    """wcs_pixel on the device against floor(p + 0.5) of astropy's pixel coordinates, every
    golden point (the nearest is 3.4e-6 px from a rounding edge, the restatement within
    1.2e-9 px of wcslib): CAR, SIN and TAN, the zenithal maps with their central row, where
    the native longitude takes its small-x form."""
    lon, lat, rx, ry = golden_points(golden, name)
    w, ws = map_wcs(dict(crval=crval, cdelt=cdelt, crpix=crpix, ctype=ctype, nx=nx, ny=ny))
    ws.galactic = 0          # the golden points of car_gal are galactic already: the projection alone
    qx, qy = np.floor(rx + 0.5), np.floor(ry + 0.5)
    qx[(qx < 0) | (qx > nx - 1)] = np.nan
    qy[(qy < 0) | (qy > ny - 1)] = np.nan
    ref = qy * nx + qx
    ref[np.isnan(ref)] = -1
    ref = ref.astype(int)
    assert (ref >= 0).sum() > 1000 and (ref < 0).sum() > 100
    if name in ('sin', 'tan'):
        assert np.sum(np.abs(native_x(w, lon, lat)) < 1e-5) >= 60
    rc, msg, got = gather(one_row(lon, lat), ws)
    assert rc == 0, msg
    bad = np.flatnonzero(got['pix'][0] != ref)
    assert bad.size == 0, (name, bad[:10], got['pix'][0][bad[:10]], ref[bad[:10]])


# ---------------------------------------------------------------- (b) galactic rotation first
@pytest.mark.parametrize('name,crval,cdelt,crpix,ctype,nx,ny,tol', MAPS[3:], ids=[m[0] for m in MAPS[3:]])
def test_device_galactic_rotation_before_zenithal(golden, name, crval, cdelt, crpix, ctype, nx, ny, tol):
    """GLON-SIN / GLON-TAN: the golden (l, b) rotated to (ra, dec) on the host, then the device's
    Rotator(coord=['C','G']) + projection against the host chain on the same (ra, dec)."""
    l, b, _, _ = golden_points(golden, name)
    th, ph = astro.Rotator(coord=['C', 'G'], inv=True)((90 - b) * np.pi / 180., l * np.pi / 180.)
    ra, dec = ph * 180. / np.pi, (np.pi / 2 - th) * 180. / np.pi
    gtype = ['GLON-' + ctype[0][-3:], 'GLAT-' + ctype[1][-3:]]
    w, ws = map_wcs(dict(crval=crval, cdelt=cdelt, crpix=crpix, ctype=gtype, nx=nx, ny=ny))
    assert ws.galactic == 1
    gb, gl = astro.Rotator(coord=['C', 'G'])((90 - dec) * np.pi / 180., ra * np.pi / 180.)     # COMAPData.py:411-415
    xc, yc = gl * 180. / np.pi, (np.pi / 2 - gb) * 180. / np.pi
    ref = transform_to_1d(xc, yc, w, nx, ny)
    px, py = w.wcs_world2pix(xc, yc, 0)
    edge = np.minimum(np.abs(px + 0.5 - np.round(px + 0.5)), np.abs(py + 0.5 - np.round(py + 0.5)))
    print(f'{name}: nearest rounding edge {edge.min():.3g} px')
    assert edge.min() >= 1e-6
    assert (ref >= 0).sum() > 1000 and (ref < 0).sum() > 100
    rc, msg, got = gather(one_row(ra, dec), ws)
    assert rc == 0, msg
    bad = np.flatnonzero(got['pix'][0] != ref)
    assert bad.size == 0, (name, bad[:10], got['pix'][0][bad[:10]], ref[bad[:10]])


# ---------------------------------------------------------------- (c) non-finite pointing
def trig_close(got, want):
    """The project's bound for the Sun-centric leaves (test_comapdata.check_outputs)."""
    return np.max(np.abs(got - want)) <= 1e-12 * max(np.max(np.abs(want)), 1.0)


def test_nonfinite_pointing(golden):
    """NaN / +-inf in ra only, in dec only and in both: pixel -1; the Sun rotation is skipped and
    the non-finite value goes through the haversine (astro.sun_distance_deg); NaN < 10 is false,
    so the Sun cut leaves the weight alone; tod and the other columns are untouched."""
    mjd = float(golden['suncut_mjd'][1])
    sra, sdec = astro.sun_radec(mjd)
    rng = np.random.default_rng(3)
    T = 90
    ra = sra + rng.uniform(20, 60, T)            # far from the Sun: no finite sample is cut either
    dec = sdec + rng.uniform(-5, 5, T)
    nf = [np.nan, np.inf, -np.inf]
    where = {}
    for i, v in enumerate(nf):
        ra[3 + i] = v
        dec[13 + i] = v
        ra[23 + i], dec[23 + i] = v, nf[(i + 1) % 3]
        ra[33 + i], dec[33 + i] = v, v
    for s in (3, 13, 23, 33):
        where.update({s + i: 1 for i in range(3)})
    bad = np.array(sorted(where))
    t = one_row(ra, dec, chunk=9, sun_rot=astro.Rotator(rot=[sra, sdec], inv=True).mat)
    t['tod'] = rng.standard_normal((1, 1, T))
    t['az'], t['el'] = rng.uniform(0, 360, (1, T)), rng.uniform(30, 80, (1, T))
    m = dict(crval=[sra + 40, sdec], cdelt=[-0.5, 0.5], crpix=[100, 100], ctype=['RA---CAR', 'DEC--CAR'],
             nx=200, ny=200)
    w, ws = map_wcs(m)
    rc, msg, got = gather(t, ws)
    assert rc == 0, msg
    with np.errstate(invalid='ignore'):
        want_ra, want_dec = astro.sun_distance_deg(ra, dec, mjd)
        want_pix = transform_to_1d(ra, dec, w, m['nx'], m['ny'])
    fin = np.setdiff1d(np.arange(T), bad)
    assert np.all(want_pix[bad] == -1) and np.all(want_pix[fin] >= 0)
    assert np.array_equal(got['pix'][0], want_pix)
    assert np.all(np.isnan(want_ra[bad])) and np.all(want_ra[fin] >= 10)
    assert np.array_equal(got['ra'][0][bad], want_ra[bad], equal_nan=True)
    assert np.array_equal(got['dec'][0][bad], want_dec[bad], equal_nan=True)
    assert trig_close(got['ra'][0][fin], want_ra[fin]) and trig_close(got['dec'][0][fin], want_dec[fin])
    assert np.array_equal(got['w'][0, 0], np.ones(T))
    assert np.array_equal(got['tod'][0, 0], t['tod'][0, 0])
    assert np.array_equal(got['az'][0], t['az'][0]) and np.array_equal(got['el'][0], t['el'][0])
    assert np.all(got['feedid'] == 7) and np.all(got['obsid'] == 12345)


# ---------------------------------------------------------------- (d) the Sun cut at 10 degrees
def test_sun_cut_at_its_boundary(golden):
    """Points 1e-6 .. 1e-2 deg either side of the 10-degree cut around astropy's Sun at six dates:
    the device's weight mask equals dist < 10 of the host chain on every point, its distance and
    colatitude sit within the bound for these leaves."""
    rng = np.random.default_rng(11)
    worst = 0.0
    for k in range(len(golden['suncut_mjd'])):
        sra, sdec = golden['suncut_sun_ra'][k], golden['suncut_sun_dec'][k]
        ra, dec = _points_near_cut(sra, sdec, rng)
        rot = astro.Rotator(rot=[sra, sdec], inv=True)
        th, ph = rot(np.pi / 2.0 - dec * np.pi / 180.0, ra * np.pi / 180.0)
        want = astro.haversine(0, 0, ph, th) * 180.0 / np.pi
        assert (want < 10).any() and (want >= 10).any()
        assert np.min(np.abs(want - 10)) > 1e-7 and np.sum(np.abs(want - 10) < 1e-4) >= 30
        rc, msg, got = gather(one_row(ra, dec, chunk=9, sun_rot=rot.mat), map_wcs(WORLD)[1])
        assert rc == 0, msg
        assert np.array_equal(got['w'][0, 0] == 0, want < 10)
        assert np.array_equal(got['w'][0, 0], np.where(want < 10, 0.0, 1.0))
        err = max(np.max(np.abs(got['ra'][0] - want)), np.max(np.abs(got['dec'][0] - th)))
        worst = max(worst, err)
        print(f'suncut {k}: max |distance - ref| {np.max(np.abs(got["ra"][0] - want)):.3g} deg, '
              f'max |colatitude - ref| {np.max(np.abs(got["dec"][0] - th)):.3g} rad')
        assert trig_close(got['ra'][0], want) and trig_close(got['dec'][0], th)
    print(f'Sun-centric leaves, device - NumPy, maximum over the six dates: {worst:.3g}')


# ---------------------------------------------------------------- (e), (f) scan table and cuts
SCAN_CYCLE = (0, 30, 70, 10, 150, 0, 350)
# (n_scans, leading zero-length scans put in front, position in the cycle of the next scan)
SCAN_CASES = [(1, 0, 1), (2, 0, 0), (127, 0, 1), (128, 0, 4), (129, 2, 1), (300, 0, 0)]


def exact_sun_pointing(rng, F, T):
    """ra = 0, dec = +-90: Sun distance exactly 180 / 0 under EXACT_ROT (module docstring)."""
    return np.zeros((F, T)), np.where(rng.random((F, T)) < 0.8, 90.0, -90.0)


def off_edge_pointing(rng, F, T):
    """Generic (ra, dec) on the WORLD map, each at least 0.1 px from the floor(p + 0.5) edges of
    its 1-degree pixels (the pixel tests above are the ones that go near the edges)."""
    return (rng.integers(-170, 171, (F, T)) + rng.uniform(-0.4, 0.4, (F, T)),
            rng.integers(-85, 86, (F, T)) + rng.uniform(-0.4, 0.4, (F, T)))


def scan_case(n_scans, lead, k0):
    rng = np.random.default_rng(1000 * n_scans + k0)
    L = 10
    lens = ([0] * lead + [SCAN_CYCLE[(i + k0) % 7] for i in range(n_scans)])[:n_scans]
    edges, at = [], 4
    for i, n in enumerate(lens):
        extra = (3 * i) % L                  # (end - start) // L * L = n: the scan's tail is not read
        edges.append([at, at + n + extra])
        at += n + extra + (i % 3)
    T = at + 5
    F = 6                                    # file rows 0-2 feed the Sun columns, 3-5 the pixels
    ra, dec = exact_sun_pointing(rng, F, T)
    ra[3:], dec[3:] = off_edge_pointing(rng, 3, T)
    t = dict(tod=rng.standard_normal((F, 2, T)), az=rng.uniform(0, 360, (F, T)), el=rng.uniform(30, 80, (F, T)),
             ra=ra, dec=dec, spike=(rng.random((F, 2, T)) < 0.05).astype(np.uint8), edges=edges, L=L,
             row_src=[2, 0, 1], pix_src=[3, 5, 4], row_feed=[11, 3, 19], row_cal=rng.uniform(0.5, 2, (3, 4)),
             row_w=rng.uniform(0.5, 2, (3, 4)), row_pct=[[36, 324, 35, 75]] * 3, bands=(1, 0), sun_rot=EXACT_ROT,
             obsid=4242)
    return t, lens


def world_pixels(t):
    w, ws = map_wcs(WORLD)
    for ps in t['pix_src']:
        if ps >= 0:          # the restatement is within 1.2e-9 px of wcslib: stay clear of rounding edges
            px, py = w.wcs_world2pix(t['ra'][ps], t['dec'][ps], 0)
            assert np.min(np.abs(px + 0.5 - np.round(px + 0.5))) > 1e-6
            assert np.min(np.abs(py + 0.5 - np.round(py + 0.5))) > 1e-6
    return ws, lambda x, y: transform_to_1d(x, y, w, WORLD['nx'], WORLD['ny'])


def check_exact_sun(want):
    live = want['feedid'] != 0
    assert set(np.unique(want['ra'][live])) == {0.0, 180.0}
    assert set(np.unique(want['dec'][live])) == {0.0, np.pi}


def check_scan_case(n_scans, lead, k0):
    t, lens = scan_case(n_scans, lead, k0)
    ws, pixel_of = world_pixels(t)
    want = reference_file(t, pixel_of)
    check_exact_sun(want)
    assert want['az'].shape == (3, sum(lens)) and np.any(want['w'] != 0) and np.any(want['pix'] >= 0)
    rc, msg, got = gather(t, ws)
    assert rc == 0, msg
    assert_columns_equal(got, want, ('scans', n_scans))


def test_scan_cases_cover_the_edges():
    lens = {c[0]: scan_case(*c)[1] for c in SCAN_CASES}
    assert 128 in lens and 129 in lens and 128 <= K_SCAN_LDS < 129          # either side of the LDS table
    assert lens[129][:2] == [0, 0] and lens[129][2] > 0                       # two leading zero-length scans
    assert lens[128][-1] == 0 and lens[2][0] == 0 and lens[300][-1] == 0      # a trailing / a leading one
    assert any(sum(v) % 256 for v in lens.values())
    assert {n for v in lens.values() for n in v} == set(SCAN_CYCLE)


@pytest.mark.parametrize('n_scans,lead,k0', SCAN_CASES, ids=[str(c[0]) for c in SCAN_CASES])
def test_scan_table(n_scans, lead, k0):
    """Column -> (scan, sample) through the scan table, in LDS up to 128 scans and searched in
    global memory beyond, with zero-length scans in front, inside and behind."""
    check_scan_case(n_scans, lead, k0)


CUT_BANDS = [(2,), (3, 0), (0, 1, 2, 3), (3, 2, 1, 0)]


def cuts_case(bands):
    """Four output rows over scans of N = 10, 30, 70, 150, 350 (L = 10): a live row, a bad row
    whose pixels are still read, a live row without pixels, a live row whose pixels come from
    another file row; az / el on and one ulp outside the percentile band; a spike mask with
    strides of its own."""
    rng = np.random.default_rng(sum(10 ** i * b for i, b in enumerate(bands)) + 5)
    L, F, B = 10, 6, 4
    edges, at = [], 3
    for i, n in enumerate((10, 30, 70, 150, 350)):
        edges.append([at, at + n + 2 * i + 1])
        at += n + 2 * i + 1 + i % 2
    T = at + 2
    ra, dec = exact_sun_pointing(rng, F, T)
    ra[4:], dec[4:] = off_edge_pointing(rng, 2, T)
    pct = np.array([[2.0, 8.0, 40.0, 47.5]] * 4)
    lo = lambda v: np.nextafter(v, -np.inf)          # noqa: E731
    hi = lambda v: np.nextafter(v, np.inf)           # noqa: E731
    az = rng.integers(0, 21, (F, T)) * 0.5           # many samples equal to 2.0 and 8.0
    el = 38.0 + rng.integers(0, 24, (F, T)) * 0.5    # ... and to 40.0 and 47.5
    for f in range(F):
        s = rng.permutation(T)
        az[f, s[:8]], az[f, s[8:16]], az[f, s[16:24]], az[f, s[24:32]] = 2.0, lo(2.0), 8.0, hi(8.0)
        el[f, s[32:40]], el[f, s[40:48]], el[f, s[48:56]], el[f, s[56:64]] = 40.0, lo(40.0), 47.5, hi(47.5)
        az[f, s[64:68]], el[f, s[68:72]] = np.nan, np.nan            # NaN compares false: kept
    spike = np.zeros((F, B + 1, T + 13), dtype=np.uint8)
    spike[:, :B, :T] = rng.random((F, B, T)) < 0.1
    spike[:, B, :], spike[:, :, T:] = 1, 1                           # read only with the tod's strides
    t = dict(tod=rng.standard_normal((F, B, T)), az=az, el=el, ra=ra, dec=dec, spike=spike, edges=edges, L=L,
             row_src=[0, -1, 2, 1], pix_src=[0, 4, -1, 5], row_feed=[1, 0, 12, 5],
             row_cal=rng.uniform(0.5, 2, (4, 4)), row_w=rng.uniform(0.5, 2, (4, 4)), row_pct=pct, bands=bands,
             sun_rot=EXACT_ROT, obsid=99)
    return t


def check_cuts_case(bands):
    t = cuts_case(bands)
    ws, pixel_of = world_pixels(t)
    want = reference_file(t, pixel_of)
    check_exact_sun(want)
    rs = t['row_src']
    w0 = want['w'][0]
    assert np.all(want['pix'][1] >= 0) and all(np.all(want[k][..., 1, :] == 0) for k in COLS if k not in ('pix', 'obsid'))
    assert np.all(want['pix'][2] == 0) and np.any(want['w'][:, 2] != 0)
    for row in (0, 2, 3):       # on the percentile: kept somewhere; one ulp outside: present, and always cut
        for col, lohi in (('az', (2.0, 8.0)), ('el', (40.0, 47.5))):
            v = want[col][row]
            for p, out in zip(lohi, (np.nextafter(lohi[0], -np.inf), np.nextafter(lohi[1], np.inf))):
                assert np.any((v == p) & (w0[row] != 0)) and np.any(v == out) and np.all(w0[row][v == out] == 0)
    assert len({tuple(want['w'][k, 0] != 0) for k in range(len(bands))}) == len(bands)      # spikes differ per band
    assert rs[3] != t['pix_src'][3]
    rc, msg, got = gather(t, ws)
    assert rc == 0, msg
    assert_columns_equal(got, want, ('cuts', bands))


@pytest.mark.parametrize('bands', CUT_BANDS, ids=['-'.join(map(str, b)) for b in CUT_BANDS])
def test_per_sample_cuts(bands):
    check_cuts_case(bands)


# ---------------------------------------------------------------- (g), (h)
def test_healpix_ids_and_null_wcs():
    t, _ = scan_case(2, 0, 3)
    rng = np.random.default_rng(9)
    ds = int(scan_table(t['edges'], t['L'])[:, 1].sum())
    pixels = rng.integers(0, 12 * 4096 ** 2, (3, ds)).astype(np.int64)
    pixels[0, :4] = [0, 2 ** 24 + 1, 12 * 4096 ** 2 - 1, 2 ** 24 - 1]
    assert np.sum(pixels > 2 ** 24) > ds
    want = reference_file(t, pixels=pixels)
    rc, msg, got = gather(t, None, pixels=pixels)
    assert rc == 0, msg
    assert_columns_equal(got, want, 'healpix')
    assert np.array_equal(got['pix'], pixels.astype(np.int32))
    rc, _, _ = gather(t, None)
    assert rc != 0


def test_refusals():
    t, _ = scan_case(2, 0, 3)
    ws, _ = world_pixels(t)
    for override, text in ((dict(n_scans=0), 'no scan in the file'), (dict(n_bands=0), '1 to 4 bands'),
                           (dict(n_bands=5), '1 to 4 bands'), (dict(n_rows=65536), 'too many rows')):
        rc, msg, got = gather(t, ws, **override)
        assert rc != 0 and text in msg, (override, rc, msg)
        assert all(_untouched(got[k]) for k in COLS), override
    for override in (dict(n_rows=0), dict(datasize=0)):
        rc, msg, got = gather(t, ws, **override)
        assert rc == 0, (override, msg)
        assert all(_untouched(got[k]) for k in COLS), override


# ---------------------------------------------------------------- comap_prep_cut
ROW_COLS = ('az', 'el', 'ra', 'dec', 'feedid', 'obsid', 'pix')


def cut(cols, nb, n, L, in_stride, out_stride, cap):
    """One comap_prep_cut call.  cols: tod / w [nb, n], the others [n].  Returns (rc, message,
    n_kept, outputs [.., cap * L], keep_out [nb, cap], the input tod / w after the call)."""
    torch, N, dev, c = _ctx()
    from comapreduce_amd.mapmaking.prep import PrepOut
    f8 = torch.float64
    dt = lambda k: torch.int64 if k in ('feedid', 'obsid') else torch.int32 if k == 'pix' else f8     # noqa: E731
    i = {}
    for k in ('tod', 'w'):
        i[k] = torch.full((nb, in_stride), F8_SENTINEL, dtype=f8, device=dev)
        i[k][:, :n] = torch.as_tensor(cols[k], device=dev)
    for k in ROW_COLS:
        i[k] = torch.as_tensor(np.ascontiguousarray(cols[k]), device=dev).to(dt(k))
    o = {k: _fresh(torch, N, dev, (nb, out_stride) if k in ('tod', 'w') else max(cap * L, 1), dt(k)) for k in COLS}
    keep = _fresh(torch, N, dev, (nb, max(cap, 1)), torch.uint8)
    d = N.dptr
    pi, po = (PrepOut(d(a['tod']), d(a['w']), s, d(a['az']), d(a['el']), d(a['ra']), d(a['dec']), d(a['feedid']),
                      d(a['obsid']), d(a['pix']), 0) for a, s in ((i, in_stride), (o, out_stride)))
    nk = ctypes.c_int64(-5)
    rc = N.lib().comap_prep_cut(c, ctypes.byref(pi), nb, n, L, ctypes.byref(po), d(keep), cap, ctypes.byref(nk))
    torch.cuda.synchronize(dev)
    msg = N.lib().comap_last_error(c).decode() if rc else ''
    assert all(bool(torch.all(i[k][:, n:] == F8_SENTINEL)) for k in ('tod', 'w'))      # nothing past n is touched
    return (rc, msg, int(nk.value), {k: v.cpu().numpy() for k, v in o.items()}, keep.cpu().numpy(),
            {k: i[k][:, :n].cpu().numpy() for k in ('tod', 'w')})


def reference_cut(cols, nb, L):
    """COMAPData.py:550-568 per band (keep[b] = that band's own offset mask), the kept set their
    union, compacted in order.  Returns (outputs, keep [nb, kept], masked input tod / w)."""
    tod, w = cols['tod'].copy(), cols['w'].copy()
    keep = np.zeros((nb, tod.shape[1] // L), dtype=bool)
    for b in range(nb):
        mask = ~np.isfinite(tod[b])
        tod[b][mask] = 0
        w[b][mask] = 0
        zero_mask = (w[b] != 0).astype(float)
        keep[b] = np.sum(zero_mask.reshape((zero_mask.size // L, L)), axis=1) != 0
    kept = keep.any(axis=0)
    sel = np.repeat(kept, L)
    out = {k: cols[k][sel] for k in ROW_COLS}
    out['tod'], out['w'] = tod[:, sel], w[:, sel]
    out['w'][~np.isfinite(out['w'])] = 0
    return out, keep[:, kept].astype(np.uint8), {'tod': tod, 'w': w}


CUT_SHAPES = [(1, 1001, 1), (1, 5, 3), (7, 1, 4), (7, 4, 3), (64, 3, 1), (64, 1001, 4), (65, 5, 4), (65, 4, 1),
              (130, 3, 3), (130, 1, 4), (130, 5, 4)]


def cut_case(L, NO, nb):
    rng = np.random.default_rng(10000 * L + 10 * NO + nb)
    n = L * NO
    tod = rng.standard_normal((nb, n))
    w = rng.uniform(0.5, 2.0, (nb, n))
    w[rng.random((nb, n)) < 0.3] = 0.0
    w[rng.random((nb, n)) < 0.05] = -0.0
    w = w.reshape(nb, NO, L)
    w[rng.random((nb, NO)) < 0.5] = 0.0              # empty (band, offset) pairs: some offsets empty in every band
    nf = [np.nan, np.inf, -np.inf]
    # the first offsets, as far as NO goes, each hold one special content
    special = ['last sample only', 'non-finite weights only', 'band 2 only', 'minus zeros', 'weight under a NaN tod']
    for o, what in enumerate(special[:NO]):
        w[:, o] = 0.0
        if what == 'last sample only':
            w[0, o, L - 1] = 1.5
        elif what == 'non-finite weights only':
            for b in range(nb):
                w[b, o, (b * 3) % L], w[b, o, L - 1], w[b, o, L // 2] = nf[b % 3], nf[(b + 1) % 3], nf[(b + 2) % 3]
        elif what == 'band 2 only' and nb > 2:
            w[2, o, L // 3] = 0.75
        elif what == 'minus zeros':
            w[:, o] = -0.0
        elif what == 'weight under a NaN tod':
            w[:, o, L - 1] = 2.0
    w = w.reshape(nb, n)
    tod[rng.random((nb, n)) < 0.03] = np.nan
    tod[rng.random((nb, n)) < 0.01] = np.inf
    tod[rng.random((nb, n)) < 0.01] = -np.inf
    t3 = tod.reshape(nb, NO, L)
    for o, what in enumerate(special[:NO]):
        if what in ('last sample only', 'band 2 only', 'non-finite weights only'):
            t3[:, o] = rng.standard_normal((nb, L))          # finite: the special weight decides
        elif what == 'weight under a NaN tod':
            t3[:, o, L - 1] = nf[o % 3]
    for j, v in zip((0, 63, 64, 70, 127, 128, 129), nf * 3):  # non-finite tod over a live weight, second and third trips
        if j < L:
            o = NO - 1
            t3[nb - 1, o, j] = v
            w.reshape(nb, NO, L)[nb - 1, o, j] = 1.25
    cols = dict(tod=tod, w=w, az=rng.uniform(0, 360, n), el=rng.uniform(30, 80, n), ra=rng.uniform(10, 180, n),
                dec=rng.uniform(0, np.pi, n), feedid=rng.integers(1, 20, n), obsid=rng.integers(1, 2 ** 40, n),
                pix=rng.integers(-1, 2 ** 30, n).astype(np.int32))
    return cols, special[:NO]


def check_cut_shape(L, NO, nb):
    cols, special = cut_case(L, NO, nb)
    n = L * NO
    want, keep, masked = reference_cut(cols, nb, L)
    nk = keep.shape[1]
    k0 = np.zeros((nb, NO), dtype=bool)
    for b in range(nb):
        k0[b] = (masked['w'][b].reshape(NO, L) != 0).any(axis=1)
    kept = k0.any(axis=0)
    for o, what in enumerate(special):
        if what in ('last sample only', 'non-finite weights only'):
            assert kept[o]
        elif what == 'band 2 only' and nb > 2:
            assert kept[o] and list(k0[:, o]) == [False, False, True] + [False] * (nb - 3)
        elif what in ('minus zeros', 'weight under a NaN tod'):
            assert not kept[o]
    if 'non-finite weights only' in special:
        o = int(np.cumsum(kept)[1]) - 1
        assert np.all(want['w'][:, o * L:(o + 1) * L] == 0) and not np.all(np.isfinite(masked['w'][:, L:2 * L]))
    cap = nk + 3
    rc, msg, got_nk, got, got_keep, after = cut(cols, nb, n, L, n + 11, cap * L + 5, cap)
    assert rc == 0, msg
    assert got_nk == nk, (L, NO, nb)
    for k in COLS:
        g = got[k][..., :nk * L]
        assert g.dtype == want[k].dtype or k in ('feedid', 'obsid'), k
        assert np.array_equal(g, want[k], equal_nan=(k not in ('feedid', 'obsid', 'pix'))), (L, NO, nb, k)
        assert _untouched(got[k][..., nk * L:]), k
    assert np.array_equal(got_keep[:, :nk], keep) and _untouched(got_keep[:, nk:])
    for k in ('tod', 'w'):                            # the call edits its input in place
        assert np.array_equal(after[k], masked[k], equal_nan=True), (L, NO, nb, k)
    return nk


@pytest.mark.parametrize('L,NO,nb', CUT_SHAPES, ids=['-'.join(map(str, s)) for s in CUT_SHAPES])
def test_cut_vs_reference(L, NO, nb):
    """k_cut_flags (four offsets per workgroup, 64 lanes over L: one, two and three trips), the
    scan and k_cut_copy against COMAPData.py:550-568 per band."""
    check_cut_shape(L, NO, nb)


def test_cut_shapes_cover():
    for i, vals in enumerate(((1, 7, 64, 65, 130), (1, 3, 4, 5, 1001), (1, 3, 4))):
        assert all(sum(s[i] == v for s in CUT_SHAPES) >= 2 for v in vals)


def test_cut_edges():
    L, NO, nb = 7, 9, 3
    cols, _ = cut_case(L, NO, nb)
    n = L * NO
    # every offset dropped
    none = dict(cols, w=np.where(np.arange(n) % 2, 0.0, -0.0) * np.ones((nb, 1)))
    rc, msg, nk, got, keep, _ = cut(none, nb, n, L, n + 2, n + 9, NO)
    assert rc == 0 and nk == 0, msg
    assert all(_untouched(got[k]) for k in COLS) and _untouched(keep)
    # nothing dropped
    full = dict(cols, tod=np.abs(np.nan_to_num(cols['tod'], nan=1.0, posinf=2.0, neginf=3.0)), w=np.ones((nb, n)))
    rc, msg, nk, got, keep, after = cut(full, nb, n, L, n + 2, n + 9, NO)
    assert rc == 0 and nk == NO, msg
    assert all(np.array_equal(got[k][..., :n], full[k]) for k in COLS) and np.all(keep == 1)
    assert np.array_equal(after['tod'], full['tod']) and np.array_equal(after['w'], full['w'])
    # capacity one short of the kept offsets
    want, k, _ = reference_cut(cols, nb, L)
    assert k.shape[1] >= 2
    rc, msg, _, _, _, _ = cut(cols, nb, n, L, n + 2, n + 9, k.shape[1] - 1)
    assert rc != 0 and 'output capacity too small' in msg
    # a sample count that is no multiple of the offset length
    rc, msg, _, _, _, _ = cut({k: v[..., :n - 1] for k, v in cols.items()}, nb, n - 1, L, n + 2, n + 9, NO)
    assert rc != 0 and 'multiple of offset_length' in msg
    # no samples
    rc, msg, nk, got, keep, _ = cut({k: v[..., :0] for k, v in cols.items()}, nb, 0, L, 4, 9, 1)
    assert rc == 0 and nk == 0, msg
    assert all(_untouched(got[k]) for k in COLS)


# ---------------------------------------------------------------- once more under COMAP_POISON=1
def check_all_under_this_process():
    """The scan-table, per-sample-cut and cut cases, then one read_comap_data golden case: run by
    a child process under COMAP_POISON=1, where N.device_empty hands out NaN / -1 buffers."""
    for c in SCAN_CASES:
        check_scan_case(*c)
    for b in CUT_BANDS:
        check_cuts_case(b)
    for s in CUT_SHAPES:
        check_cut_shape(*s)
    import test_comapdata as TC
    store, names = TC.cc.store()
    golden = np.load(os.path.join(HERE, 'golden', 'golden_comapdata.npz'))
    case = TC.cc.CASES['car']
    res = TC.cd.read_comap_data(names, TC.map_info(case['map']), feeds=TC.cc.FEEDS, store=store, **case['kw'])
    TC.check_outputs(res, golden, 'car', device=True)


def test_gather_and_cut_under_poison():
    env = dict(os.environ, COMAP_POISON='1')
    code = ('import sys; sys.path[:0] = [%r, %r]; import test_gpu_prep_gather as T; from comapreduce_amd import _native as N; '
            'assert N.POISON; T.check_all_under_this_process(); print("poison ok")' % (os.path.dirname(HERE), HERE))
    r = subprocess.run([sys.executable, '-s', '-c', code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and 'poison ok' in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
