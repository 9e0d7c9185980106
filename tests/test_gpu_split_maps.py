"""Split maps (per-feed / per-observation maps from one destriper solve): the device pass
comap_destripe_split_maps and its path up through DeviceDestriper(split=...), run_destriper,
run_destriper_bands and run_destriper.main, against oracle.destriper.bin_offset_map on the selected
samples with the DEVICE's own offsets.  The sums are binValues' sums in sample order, every
operation rounded on its own, so weight, hits, num, naive_num and the divided maps must be equal
bit for bit (array_equal), not close.

Inputs: the cases of test_gpu_destriper_ground.py (A: every branch at the smallest size; B: 60 000
samples, the count entry form) and a pile-up case built here (one pixel row longer than any
workgroup)."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_destriper_ground import CASE_A, CASE_B, RTOL, make_case, relmax  # noqa: E402

pytestmark = pytest.mark.gpu

KEYS = ('map', 'naive', 'weight', 'hits')


# ---------------------------------------------------------------- the oracle
def oracle_split(pix, tod, w, x, L, labels, G, npix, keep=None):
    """{'num', 'naive_num', 'weight', 'hits', 'map', 'naive'}, each [G, npix]: bin_offset_map on
    the samples of each label (label[t // L] == g), z = tod - repeat(x, L); hits from its ones
    variant on the samples of kept offsets."""
    from oracle.destriper import bin_offset_map, share_map
    pix = np.asarray(pix, np.int64)
    z = tod - np.repeat(x, L)
    lab = np.repeat(np.asarray(labels), L)
    kept = np.ones(pix.size, bool) if keep is None else np.repeat(np.asarray(keep) != 0, L)
    one = np.ones(pix.size)
    out = {k: np.zeros((G, npix)) for k in ('num', 'naive_num', 'weight', 'hits', 'map', 'naive')}
    for g in range(G):
        s = lab == g
        out['num'][g], out['weight'][g] = bin_offset_map(pix[s], z[s], w[s], npix)
        out['naive_num'][g], _ = bin_offset_map(pix[s], tod[s], w[s], npix)
        out['hits'][g], _ = bin_offset_map(pix[s & kept], one[s & kept], one[s & kept], npix)
        out['map'][g] = share_map(out['num'][g], out['weight'][g])
        out['naive'][g] = share_map(out['naive_num'][g], out['weight'][g])
    return out


def raw_call(pix, tod, w, x, labels, G, L, npix, nb=1, keep=None, out_elems=None):
    """comap_destripe_split_maps itself on host inputs (tod / w [nb, N], x [N/L, nb]):
    (rc, {'num', 'naive_num', 'weight', 'hits'} as [G, npix, nb], the error text).  out_elems: the
    size of each output buffer, for calls that must fail before they touch one."""
    import torch
    from comapreduce_amd import _native as N
    dev = torch.device('cuda', N.current_device())
    c = N.ctx()
    N.bind_stream(c, dev)

    def t(a, dt):
        return torch.from_numpy(np.ascontiguousarray(a)).to(device=dev, dtype=dt).contiguous()
    args = [t(pix, torch.int32), t(tod, torch.float64), t(w, torch.float64),
            None if keep is None else t(keep, torch.uint8), t(x, torch.float64), t(labels, torch.int32)]
    out = [N.device_empty(G * npix * nb if out_elems is None else out_elems, torch.float64, dev) for _ in range(4)]
    rc = N.lib().comap_destripe_split_maps(c, *(None if a is None else N.dptr(a) for a in args), G, int(np.size(pix)),
                                           L, npix, nb, *(N.dptr(o) for o in out))
    torch.cuda.synchronize()
    msg = N.lib().comap_last_error(c).decode()
    if out_elems is not None:
        return rc, None, msg
    return rc, {k: o.cpu().numpy().reshape(G, npix, nb) for k, o in zip(('num', 'naive_num', 'weight', 'hits'), out)}, msg


def feed_labels(case):
    from comapreduce_amd.mapmaking.destriper import split_labels
    return split_labels('feed', case['feed'], case['obs'], case['L'])


def group_labels(case):
    """One label per (observation, feed) group: every offset labelled."""
    from comapreduce_amd.mapmaking.destriper import ground_groups
    gid, uobs, ufeed = ground_groups(case['feed'], case['obs'], case['L'])
    return gid, int(uobs.size * ufeed.size)


# ---------------------------------------------------------------- 1. the C call alone
def check_c_call():
    """Case A through the C entry point alone (row-major pixels, one band); also run in a child
    process under COMAP_POISON=1 (the variable is read once per process)."""
    case = make_case(**CASE_A)
    L, npix = case['L'], case['npix']
    assert L == 10 and case['pix'].size == 5 * 23 * L and npix == 144
    assert {-1, -5} <= set(case['pix'].tolist()) and 0.02 < np.mean(case['w'] == 0) < 0.09
    lab, names = feed_labels(case)
    assert len(names) == 3
    lab = lab.copy()
    lab[[7, 60]] = -1                                     # two offsets in no split
    x = np.random.default_rng(2).standard_normal(lab.size)
    for G in (3, 4):                                      # 4: a label that owns no offset
        want = oracle_split(case['pix'], case['tod'], case['w'], x, L, lab, G, npix)
        rc, got, msg = raw_call(case['pix'], case['tod'], case['w'], x, lab, G, L, npix)
        assert rc == 0, msg
        for k in ('num', 'naive_num', 'weight', 'hits'):
            assert np.array_equal(got[k][:, :, 0], want[k]), (G, k)
        assert np.all(want['hits'][:3].sum(axis=1) > 0)
        if G == 4:
            assert all(np.all(got[k][3] == 0.0) for k in got)
        rc, again, _ = raw_call(case['pix'], case['tod'], case['w'], x, lab, G, L, npix)
        assert rc == 0 and all(got[k].tobytes() == again[k].tobytes() for k in got)
    # argument and range errors
    bad = case['pix'].copy()
    bad[17] = npix
    assert raw_call(bad, case['tod'], case['w'], x, lab, 3, L, npix)[0] == -3
    bad[17] = -npix - 1
    assert raw_call(bad, case['tod'], case['w'], x, lab, 3, L, npix)[0] == -3
    for wrong in (3, -2):
        lb = lab.copy()
        lb[5] = wrong
        rc, _, msg = raw_call(case['pix'], case['tod'], case['w'], x, lb, 3, L, npix)
        assert rc != 0 and 'label' in msg
    rc, _, msg = raw_call(case['pix'], case['tod'], case['w'], x, lab, 3, L, npix, nb=3, out_elems=8)
    assert rc != 0 and 'n_bands' in msg
    rc, _, msg = raw_call(case['pix'], case['tod'], case['w'], x, lab, 2 ** 31 // npix + 1, L, npix, out_elems=8)
    assert rc != 0 and 'n_labels' in msg
    check_degenerate_segments()


def check_degenerate_segments():
    """The segment counts at their smallest (L = 10, 7 pixels, one band, one label): only the
    sentinel's segment -- through the label, then through the pixel -- exactly one live segment, and
    a single offset."""
    L, npix = 10, 7
    rng = np.random.default_rng(11)
    for what, NO, pix, label in (('all labelled -1', 3, None, -1), ('one pixel', 3, 4, 0), ('every pixel -2', 3, -2, 0),
                                 ('one offset', 1, None, 0)):
        n = NO * L
        p = rng.integers(0, npix, n).astype(np.int32) if pix is None else np.full(n, pix, np.int32)
        tod, w, x = rng.standard_normal(n), rng.uniform(0.5, 2.0, n), rng.standard_normal(NO)
        lab = np.full(NO, label, np.int32)
        want = oracle_split(p, tod, w, x, L, lab, 1, npix)
        rc, got, msg = raw_call(p, tod, w, x, lab, 1, L, npix)
        assert rc == 0, (what, msg)
        for k in ('num', 'naive_num', 'weight', 'hits'):
            assert np.array_equal(got[k][:, :, 0], want[k]), (what, k)
        if label < 0 or pix == -2:
            assert all(np.all(got[k] == 0.0) for k in got), what
        elif pix == 4:
            assert got['hits'][0, 4, 0] == n and np.count_nonzero(got['hits']) == 1, what
        else:
            assert got['hits'].sum() == n, what


def test_c_call_alone():
    check_c_call()


def test_c_call_alone_under_poison():
    env = dict(os.environ, COMAP_POISON='1')
    code = ('import sys; sys.path[:0] = [%r, %r]; import test_gpu_split_maps as T; T.check_c_call(); print("poison ok")'
            % (os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__))))
    r = subprocess.run([sys.executable, '-s', '-c', code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and 'poison ok' in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ---------------------------------------------------------------- through DeviceDestriper
def interleaved(ops, x2):
    """Host offsets [n_bands, N/L] as the operator's device vector [N/L * nb] (band fastest, a
    padded band 0)."""
    import torch
    xi = torch.zeros((ops.n_offsets, ops.nb), dtype=torch.float64, device=ops.dev)
    xi[:, :x2.shape[0]] = torch.from_numpy(np.ascontiguousarray(x2.T)).to(ops.dev)
    return xi.reshape(-1)


def solve_and_check(pix, tod, w, L, npix, labels, G, keep=None, map_shape=None, threshold=1e-6, niter=30):
    """DeviceDestriper(split=...).solve() against the oracle with the solve's own offsets; tod / w
    [N] (one band) or [n_bands, N].  Returns (res, res['splits'] on the host, raw, dd) with raw
    the C call's sums when the problem runs on the caller's pixel order (map_shape None)."""
    from comapreduce_amd.mapmaking.destriper import DeviceDestriper
    dd = DeviceDestriper(pix, tod, w, L, npix, keep=keep, map_shape=map_shape, split=(labels, G))
    res = dd.solve(threshold, niter)
    multi = np.ndim(tod) == 2
    tod2, w2 = np.atleast_2d(tod), np.atleast_2d(w)
    keep2 = None if keep is None else np.atleast_2d(keep)
    x2 = np.atleast_2d(res['x'].cpu().numpy())
    sp = {k: res['splits'][k].cpu().numpy() for k in KEYS}
    assert set(res['splits']) == set(KEYS)
    assert sp['map'].shape == ((tod2.shape[0], G, npix) if multi else (G, npix))
    raw = None
    if map_shape is None:
        ops = dd.ops
        raw = [v.cpu().numpy().reshape(G, npix, ops.nb) for v in ops.split_maps(interleaved(ops, x2), dd.split[0][0], G)]
    for b in range(tod2.shape[0]):
        want = oracle_split(pix, tod2[b], w2[b], x2[b], L, labels, G, npix, None if keep2 is None else keep2[b])
        for k in KEYS:
            got = sp[k][b] if multi else sp[k]
            assert np.array_equal(got, want[k]), (b, k, int(np.sum(got != want[k])))
        if raw is not None:
            for v, k in zip(raw, ('num', 'naive_num', 'weight', 'hits')):
                assert np.array_equal(v[:, :, b], want[k]), (b, k)
    if raw is not None and raw[0].shape[2] > tod2.shape[0]:      # the padded fourth band: nothing binned
        assert all(np.all(v[:, :, -1] == 0.0) for v in raw)
    return res, sp, raw, dd


# ---------------------------------------------------------------- 2. pile-up
@pytest.mark.parametrize('form', ['f64', 'count'])
def test_pile_up_row_longer_than_a_workgroup(form):
    rng = np.random.default_rng(8)
    n, L, npix = 4000, 50, 16
    pix = rng.integers(0, npix, n).astype(np.int32)
    pix[rng.permutation(n)[:3000]] = 5
    labels = (np.arange(n // L) % 2).astype(np.int32)
    lab_s = np.repeat(labels, L)
    for g in range(2):
        assert np.sum((pix == 5) & (lab_s == g)) >= 1024
    tod = rng.standard_normal(n)
    if form == 'f64':
        w = 0.5 + rng.random(n)                            # weights vary inside offsets
    else:
        w = np.repeat(0.5 + rng.random(n // L), L)         # one weight per offset, 5 % zeros
        w[rng.random(n) < 0.05] = 0.0
    from comapreduce_amd.mapmaking.destriper import DeviceOps
    assert DeviceOps(pix, tod, w, L, npix).entry_bytes() == (12 if form == 'f64' else 5)
    solve_and_check(pix, tod, w, L, npix, labels, 2)


def test_every_row_long():
    """32 rows of about 1250 samples each: one wave of the summing kernel holds long rows
    throughout and sums them lane by lane (the pile-up above: two long rows, summed by the wave
    together); the tail rows straddle the 512-sample threshold between the two paths."""
    rng = np.random.default_rng(9)
    n, L, npix = 40_000, 50, 18
    pix = rng.integers(0, 16, n).astype(np.int32)
    labels = (np.arange(n // L) % 2).astype(np.int32)
    lab_s = np.repeat(labels, L)
    z = np.nonzero(lab_s == 0)[0][rng.permutation(n // 2)]      # label 0's rows in pixels 16 and 17:
    pix[z[:511]], pix[z[511:1023]] = 16, 17                      # 511 and 512 samples
    rows = np.bincount(lab_s * npix + pix, minlength=2 * npix)
    assert rows[16] == 511 and rows[17] == 512 and np.sum(rows >= 512) > 8 and rows[:16].min() >= 1024
    solve_and_check(pix, rng.standard_normal(n), 0.5 + rng.random(n), L, npix, labels, 2)


@pytest.mark.parametrize('rows', ['few', 'many'])
@pytest.mark.parametrize('nb', [2, 3, 4])
def test_long_rows_with_bands_and_keep(nb, rows):
    """The long-row paths with everything the field has: several bands with their own tod and
    weights and a keep mask (10 % of the offsets dropped per band, their weights zeroed), against
    the oracle per band.  'few': the pile-up, whose two rows of about 1500 samples fall in different
    waves of the summing kernel (16 rows x 4 bands, or 32 x 2, per wave), so each wave holds at most
    8 long (row, band) lanes and sums them together -- the hit count then comes from the band's
    keep row through the wave's ballot, x and tod from the band the wave was handed.  'many': 32
    rows of about 1250 samples, long lanes throughout every wave: the lane-parallel path."""
    rng = np.random.default_rng(100 + nb)
    L = 50
    if rows == 'few':
        n, npix = 4000, 16
        pix = rng.integers(0, npix, n).astype(np.int32)
        pix[rng.permutation(n)[:3000]] = 5
    else:
        n, npix = 40_000, 16
        pix = rng.integers(0, npix, n).astype(np.int32)
    labels = (np.arange(n // L) % 2).astype(np.int32)
    count = np.bincount(np.repeat(labels, L) * npix + pix, minlength=2 * npix)
    long_rows = np.nonzero(count >= 512)[0]
    per_wave = 64 // (4 if nb == 3 else nb)               # rows per wave (3 bands run as 4)
    in_wave = np.bincount(np.searchsorted(np.nonzero(count)[0], long_rows) // per_wave) * (4 if nb == 3 else nb)
    if rows == 'few':
        assert long_rows.tolist() == [5, npix + 5] and count[5] >= 1024 and in_wave.max() <= 8
    else:
        assert long_rows.size == 32 and in_wave.min() > 8
    tod = rng.standard_normal((nb, n))
    w = 0.5 + rng.random((nb, n))
    keep = (rng.random((nb, n // L)) >= 0.1).astype(np.uint8)
    assert np.all((keep == 0).sum(axis=1) > 0) and len({k.tobytes() for k in keep}) == nb      # band-specific masks
    w = w * np.repeat(keep, L, axis=1)
    _, sp, _, _ = solve_and_check(pix, tod, w, L, npix, labels, 2, keep=keep)
    assert np.all(sp['hits'][:, :, 5] < count[[5, npix + 5]][None, :])       # dropped offsets left out of the long rows


# ---------------------------------------------------------------- 3. bands and keep
_B = {}


def case_b_bands(nb):
    """Case B as nb bands: band-specific tod and weights, 10 % of the offsets dropped per band
    (keep 0, their weights zeroed)."""
    if nb not in _B:
        case = _B.setdefault('case', make_case(**CASE_B))
        rng = np.random.default_rng(40 + nb)
        n, L = case['pix'].size, case['L']
        assert L == 50 and n // L == 1200 and case['npix'] == 64 * 64
        tod = rng.standard_normal((nb, n))
        w = case['w'][None, :] * (0.5 + rng.random((nb, 1)))
        keep = (rng.random((nb, n // L)) >= 0.1).astype(np.uint8)
        w = w * np.repeat(keep, L, axis=1)
        assert np.all((keep == 0).sum(axis=1) > 60)
        _B[nb] = (case, tod, w, keep)
    return _B[nb]


@pytest.mark.parametrize('nb', [3, 4])
def test_bands_and_keep_tiled_and_row_major(nb):
    case, tod, w, keep = case_b_bands(nb)
    labels, G = group_labels(case)
    args = (case['pix'], tod, w, case['L'], case['npix'], labels, G)
    res_t, tiled, _, dd_t = solve_and_check(*args, keep=keep, map_shape=(64, 64))
    res_r, rows, _, _ = solve_and_check(*args, keep=keep)
    for k in ('naive', 'weight', 'hits'):
        assert np.array_equal(tiled[k], rows[k]), k
    # 'map' is binned with the solve's offsets, and the two layouts' solves order their sums
    # differently (their offsets agree to rounding, not bit for bit: printed); the tiled pass on the
    # row-major solve's offsets gives the row-major maps bit for bit
    x_t, x_r = res_t['x'].cpu().numpy(), res_r['x'].cpu().numpy()
    print(f'{nb} bands: max |x tiled - x row-major| = {np.max(np.abs(x_t - x_r)):.3g} (max |x| {np.max(np.abs(x_r)):.3g})')
    # (two solves of one system whose sums run in different orders: the project's bound for that,
    # RTOL, as for the two layouts' maps in test_gpu_destriper_ground_ranks.py)
    assert relmax(x_t, x_r) <= RTOL
    again = dd_t._split_maps(interleaved(dd_t.ops, x_r))
    for k in KEYS:
        assert np.array_equal(again[k].cpu().numpy(), rows[k]), k
    # hits leave out the dropped offsets: fewer than the hits of all samples where a band dropped some
    full = np.bincount(case['pix'][case['pix'] >= 0], minlength=case['npix'])
    assert np.all(rows['hits'].sum(axis=1) <= full) and np.all(rows['hits'].sum(axis=(1, 2)) < full.sum())


# ---------------------------------------------------------------- 4. consistency with 'All'
def test_labels_add_up_to_all():
    case, tod, w, keep = case_b_bands(3)
    labels, G = group_labels(case)
    assert np.all(labels >= 0)
    res, sp, raw, _ = solve_and_check(case['pix'], tod[0], w[0], case['L'], case['npix'], labels, G, keep=keep[:1],
                                   threshold=1e-8, niter=200)
    al = {k: res['maps'][k].cpu().numpy() for k in KEYS}
    assert np.array_equal(sp['hits'].sum(axis=0), al['hits'])
    n_max = float(al['hits'].max())
    wsum = sp['weight'].sum(axis=0)
    bound = 2 * (n_max + G) * 2.0 ** -53
    assert np.all(np.abs(wsum - al['weight']) <= bound * al['weight'])
    num = raw[0][:, :, 0].sum(axis=0)                    # the C call's raw numerators
    linked = np.where(al['weight'] != 0, num / np.where(al['weight'] != 0, al['weight'], 1.0), num)
    e = relmax(linked, al['map'])
    print(f'relmax sum_g num_g / weight vs All map: {e:.3g}; max |sum weight - All| / All '
          f"{np.max(np.abs(wsum - al['weight']) / np.maximum(al['weight'], 1e-300)):.3g} (bound {bound:.3g})")
    assert e <= RTOL


# ---------------------------------------------------------------- 5. off means off
def test_off_means_off_and_errors():
    from comapreduce_amd.mapmaking.destriper import DeviceDestriper, run_destriper
    case = make_case(**CASE_A)
    args = (case['pix'], case['tod'], case['w'], case['L'], case['npix'])
    r0 = DeviceDestriper(*args).solve(1e-6, 100)
    r1 = DeviceDestriper(*args, split=None).solve(1e-6, 100, to_host=True)
    assert 'splits' not in r0 and 'splits' not in r1 and set(r0) == {'x', 'iters', 'maps'}
    edges = np.arange(case['npix'])
    out = run_destriper(*args[:4], edges, feedid=case['feed'], obsids=case['obs'])
    assert set(out) == {'All'} and set(out['All']) == {'map', 'naive', 'weight', 'hits', 'map2'}
    lab, names = feed_labels(case)
    with pytest.raises(NotImplementedError):
        DeviceDestriper(*args, ground=(case['az'], case['feed'], case['obs']), split=(lab, len(names)))
    with pytest.raises(NotImplementedError):
        run_destriper(*args[:4], edges, az=case['az'], feedid=case['feed'], obsids=case['obs'], ground=True,
                      split='feed')
    with pytest.raises(ValueError):
        DeviceDestriper(*args, split=(lab, len(names) - 1))              # a label >= n_labels (host labels)
    import torch
    dd = DeviceDestriper(*args, split=(torch.from_numpy(lab).cuda(), len(names) - 1))
    with pytest.raises(ValueError):
        dd.solve(1e-6, 10)                                               # device labels: the pass reports it
    bad = case['pix'].copy()
    bad[3] = case['npix']
    with pytest.raises(IndexError):
        DeviceDestriper(bad, *args[1:], split=(lab, len(names)))
    # the driver's names and the to_host path (host arrays, the same bits as the device maps)
    out = run_destriper(*args[:4], edges, feedid=case['feed'], obsids=case['obs'], split=['feed', 'obsid'])
    assert set(out) == {'All', 'offsets', 'Feed01', 'Feed04', 'Feed07', 'Obs100', 'Obs107'}
    want = oracle_split(case['pix'], case['tod'], case['w'], out['offsets'], case['L'], lab, 3, case['npix'])
    for g, name in enumerate(names):
        assert set(out[name]) == set(KEYS) and isinstance(out[name]['map'], np.ndarray)
        for k in KEYS:
            assert np.array_equal(out[name][k], want[k][g]), (name, k)


# ---------------------------------------------------------------- 6. the driver
def test_main_writes_split_maps(tmp_path):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
    import comapdata_case as cc
    from comapreduce_amd.mapmaking import comapdata as CD
    from comapreduce_amd.mapmaking.destriper import split_labels
    from comapreduce_amd.mapmaking.fits import read_image_hdus
    from comapreduce_amd.mapmaking.run_destriper import main
    store, names = cc.store()
    m = cc.CASES['car']['map']
    geo = dict(nxpix=m['nxpix'], nypix=m['nypix'], crval=m['crval'], crpix=m['crpix'], ctype=m['ctype'],
               cdelt=m['cdelt'])
    kw = dict(offset_length=50, prefix='t', feeds=cc.FEEDS, use_gain_filter=True, calibration=False, threshold=1e-6,
              niter=50, bands=(0, 1), store=store, split=['feed', 'obsid'], **geo)
    runs = {}
    for mode, batch in (('batched', True), ('per_band', False)):
        runs[mode] = main(names[:2], output_dir=str(tmp_path / mode), batch_bands=batch, **kw)
        for b in (0, 1):
            for name in ('All', 'Feed01', 'Feed02', 'Feed03', 'Feed04', 'Obs12', 'Obs13'):
                hdus = read_image_hdus(str(tmp_path / mode / f'{name}_t_Band{b:02d}.fits'))
                assert len(hdus) == 4, (mode, name, b)
                assert np.array_equal(hdus[0][1].ravel(), runs[mode][b][name]['map'], equal_nan=True)
                assert np.array_equal(hdus[3][1].ravel(), runs[mode][b][name]['hits'])
    mi = CD.map_info_from(m['crval'], m['cdelt'], m['crpix'], m['ctype'], m['nxpix'], m['nypix'])
    npix = m['nxpix'] * m['nypix']
    for b in (0, 1):
        out = runs['per_band'][b]
        tod, w, pix, _, _, _, _, _, feedid, obsids = CD.read_comap_data(names[:2], mi, iband=b, offset_length=50,
                                                                       feeds=cc.FEEDS, store=store)
        lab, lnames = split_labels('feed', feedid, obsids, 50)
        g = lnames.index('Feed02')
        want = oracle_split(pix, tod, w, out['offsets'], 50, lab, len(lnames), npix)
        assert want['hits'][g].sum() > 0
        for k in KEYS:
            assert np.array_equal(out['Feed02'][k], want[k][g]), (b, k)
        # the batched solve (dropped offsets kept with zero weight) against the per-band one, as for 'All':
        # the sums that do not depend on the offsets are equal, the map agrees within 1e-6 of its scale
        for name in ('Feed01', 'Feed02', 'Feed03', 'Feed04', 'Obs12', 'Obs13'):
            one, bat = out[name], runs['batched'][b][name]
            for k in ('weight', 'hits', 'naive'):
                assert np.array_equal(bat[k], one[k]), (b, name, k)
            fin = one['weight'] > 0
            if np.any(fin):
                assert np.max(np.abs(bat['map'][fin] - one['map'][fin])) <= 1e-6 * np.max(np.abs(one['map'][fin]))
