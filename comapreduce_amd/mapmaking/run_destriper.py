"""Map-making driver: mirror of reference comancpipeline/MapMaking/run_destriper.py.

    python run_destriper.py parameters.ini
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 run_destriper.py parameters.ini

One process per GPU (torch.distributed over RCCL, RANK/WORLD_SIZE from the
environment) replaces mpi4py.  The 4 sidebands together: read_comap_data_bands
(the whole data prep on the device: weights, cuts, pixel ids, the 400-sample
high-pass) -> one batched device destriper solve (per-iteration SUM all-reduce of
the map numerator across ranks) -> rank 0 writes each band's FITS maps.

Reference behaviours kept: files lacking averaged_tod/tod are dropped; the
source of the FIRST file decides calibrator mode (offset_length 250,
threshold 1); files are split in blocks of ``len // size`` per rank, so the
``len % size`` trailing files are not mapped (run_destriper.py:131-138).
"""
from __future__ import annotations

import os

import numpy as np

from . import comapdata as COMAPData
from .destriper import (_mask_check, _on_every_rank, _snr_spec, fknee_from_red_noise, run_destriper,
                        run_destriper_bands)
from .fits import read_image_hdus, write_image_hdus
from ..tools.parser import Parser, sex2deg

CALIBRATORS = COMAPData.CALIBRATORS


def _rank_size():
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized():
        return dist.get_rank(), dist.get_world_size()
    return 0, 1


def write_map(prefix, maps, map_info, output_dir, iband, postfix='', solve_mask=None):
    """run_destriper.write_map (run_destriper.py:19-50).  solve_mask (flags, one per pixel): one more
    image HDU 'SolveMask' (0 / 1) behind the others; without it the files are the reference's."""
    os.makedirs(output_dir, exist_ok=True)
    wcs, nx, ny = map_info['wcs'], map_info['nxpix'], map_info['nypix']
    cards = wcs.to_header()
    for k, v in maps.items():
        images = [(None, np.reshape(v['map'], (ny, nx)))]
        if 'naive' in v:
            images.append(('Naive', np.reshape(v['naive'], (ny, nx))))
        if 'weight' in v:
            with np.errstate(divide='ignore'):
                images.append(('Noise', np.reshape(np.sqrt(1. / v['weight']), (ny, nx))))
        if 'hits' in v:
            images.append(('Hits', np.reshape(v['hits'], (ny, nx))))
        if solve_mask is not None:
            images.append(('SolveMask', np.reshape(np.asarray(solve_mask) != 0, (ny, nx)).astype(np.float64)))
        fname = '{}/{}_{}_Band{:02d}.fits'.format(output_dir, k, prefix, iband)
        write_image_hdus(fname, images, cards)


def write_map_healpix(prefix, maps, remapping_array, map_info, output_dir, iband, postfix='', nside=4096):
    """run_destriper.write_map_healpix (run_destriper.py:53-77): per map set a
    partial HEALPix file of (map, naive, sqrt(1/weight)) on the union pixels."""
    from .healpix import UNSEEN, nside2npix, write_map_partial
    os.makedirs(output_dir, exist_ok=True)
    for k, v in maps.items():
        m = np.zeros((3, nside2npix(nside))) + UNSEEN
        m[0, remapping_array] = v['map']
        m[1, remapping_array] = v['naive']
        with np.errstate(divide='ignore'):
            m[2, remapping_array] = np.sqrt(1. / v['weight'])
        fname = '{}/{}_{}_Band{:02d}.fits'.format(output_dir, k, prefix, iband)
        write_map_partial(fname, m, nside)


def _healpix_edges(pointing):
    """run_destriper.py:159-161: pixel_edges = arange(max over ranks of pointing + 1)."""
    import torch.distributed as dist
    mx = int(np.max(pointing)) if np.size(pointing) else -1
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        import torch
        dev = torch.device('cuda', torch.cuda.current_device()) if dist.get_backend() == 'nccl' else 'cpu'
        t = torch.tensor([mx], dtype=torch.int64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        mx = int(t.item())
    return np.arange(mx + 1, dtype=int)


def _file_work(f, offset_length, feeds, map_info, healpix):
    """The CG work one file brings a rank: its operator entries -- the (offset, pixel run)
    pairs of its scan pointing (rankplan.offset_pixel_runs) -- plus FILE_KAPPA x its offsets
    (per-offset CG vector work in entries-equivalent units, as bench.py's field split)."""
    from . import rankplan
    fi, _ = COMAPData.GetFeeds(f['spectrometer/feeds'], feeds)
    datasize = int(COMAPData.countDataSize(f, len(fi), offset_length)['datasize'])
    if datasize == 0 or len(fi) == 0:
        return 0
    read = COMAPData.read_pixels_healpix if healpix else COMAPData.read_pixels
    pix = np.asarray(read(f, datasize, offset_length, feeds, map_info))[:len(fi), :datasize]
    entries = int(rankplan.offset_pixel_runs(pix.astype(np.int64), offset_length, groups=pix.shape[0]).sum())
    return entries + int(FILE_KAPPA * pix.size // offset_length)


FILE_KAPPA = 6.5


def _rank_files(filelist, rank, size, offset_length, feeds, map_info, healpix, open_file):
    """This rank's files.  The mapped set is the reference's: the first (len // size) x size
    files (run_destriper.py:131-138 drops the remainder); the reference then deals them in
    equal counts.  Here (COMAP_DS_SPLIT=work, the default) they are dealt in contiguous
    ranges balanced on each file's CG work (_file_work; every rank weighs its own
    equal-count share, the weights are all-gathered): a sharded CG iteration waits for its
    slowest rank, whose time follows its operator entries, not its file count.  The maps do
    not depend on which rank holds a file.  COMAP_DS_SPLIT=count: the reference's split."""
    step = filelist.size // size
    lo, hi = step * rank, min(step * (rank + 1), filelist.size)
    if size == 1 or step == 0 or os.environ.get('COMAP_DS_SPLIT', 'work') == 'count':
        return filelist[lo:hi]
    import torch.distributed as dist
    from . import rankplan
    mine = [_file_work(open_file(f), offset_length, feeds, map_info, healpix) for f in filelist[lo:hi]]
    parts = [None] * size
    dist.all_gather_object(parts, mine)
    weights = [w for p in parts for w in p]
    a, b = rankplan.balanced_ranges(weights, size)[rank]
    return filelist[:step * size][a:b]


def main(filelistname, offset_length=50, feed_weights=None, prefix='fg9', output_dir='maps/fg9/', obsid_cuts=[],
         feeds=[1, 2, 3, 5, 6, 9, 11, 12, 13, 14, 15, 16, 17, 18, 19], nxpix=480, nypix=480,
         crval=['05:32:00.3', '+12:30:28.0'], crpix=[240, 240], ctype=['RA---CAR', 'DEC--CAR'],
         cdelt=[-0.016666, 0.016666], use_gain_filter=True, calibration=True, calibrator='TauA', threshold=1e-6,
         niter=100, healpix=False, bands=(0, 1, 2, 3), store=None, device=None, batch_bands=True, ground=False,
         split=None, residuals=False, residual_cut=None, noise_prior=None, solve_mask=None):
    """run_destriper.main (run_destriper.py:79-189).  ``store`` (tests) maps
    filename -> (datasets, attrs) instead of reading files; ``device`` is the
    rank's GPU (default: torch's current device, LOCAL_RANK under torchrun).
    ``batch_bands``: the bands share the pointing, so they are read with one
    batched median call and solved as ONE batched device system
    (read_comap_data_bands + run_destriper_bands); False runs the reference's
    per-band loop.  The maps are the same either way.
    ``ground`` ([Inputs] ground_template in the .ini, absent = False): also fit an azimuth
    slope and a level per (observation, feed) jointly with the offsets (the reference's
    op_Ax_with_ground, Destriper.py:265-336, which its run() leaves switched off).  This
    takes the per-band loop, which reads az / feedid / obsids; rank 0 writes each band's fit
    -- across ranks the merged table of all ranks' observations -- to
    <output_dir>/<prefix>_ground_band<iband>.npz and the band's entry gains 'Ground' (None on
    the other ranks).  Files are whole observations, so each (observation, feed) lies on the
    one rank that holds the file.
    ``split`` ([Inputs] split_maps in the .ini: feed, obsid or both; absent = none): also map
    every feed ('Feed01', ...) and / or observation ('Obs<obsid>') on its own, from its samples of
    tod - F x with the solve's offsets (the reference's commented "Create individual feed maps
    too" block, Destriper.py:487-501): each band's dict gains one entry per name and rank 0
    writes <name>_<prefix>_Band<iband>.fits beside All_...; the band's dict also keeps 'offsets',
    the rank's solved offsets the split maps were binned with.  Not together with ``ground``.
    ``residuals`` / ``residual_cut`` ([Inputs] residual_chi2 and residual_cut in the .ini; absent =
    off): the residual chi-squared of tod - F x - P m per (observation, feed) and, with a cut c,
    one more solve without the (observation, feed) groups whose chi-squared is not <= c
    (destriper.run_destriper); each band's entry gains 'Residuals' (None on ranks other than 0)
    and rank 0 writes <output_dir>/<prefix>_residuals_band<iband>.npz.  ``chi2_cutoff`` and
    ``obsid_cuts`` stay ignored, as in the reference.  Not together with ``ground``.
    ``noise_prior`` ([Inputs] noise_prior in the .ini; absent = off): a noise prior on the offsets
    (destriper.run_destriper's ``prior``) -- (fknee, alpha[, taps]) applies one model to every
    (observation, feed); 'fnoise' takes each file's ``fnoise_fits/fnoise_fit_parameters`` (the
    Level-2 red-noise fits): per (file, feed, band) the medians of fknee and alpha over the scans
    with a valid fit, no prior for a group without one, ValueError for a file without the dataset.
    This takes the per-band loop, as ``ground`` does; the files written are the same.  Not together
    with ``ground``.
    ``solve_mask`` ([Inputs] solve_mask in the .ini; absent = off): fit the offsets from the samples
    outside a pixel mask and bin the maps from every sample (destriper.run_destriper's
    ``solve_mask``).  A path names a FITS file whose first image HDU, (nypix, nxpix), is the mask
    (non-zero = masked; NaN is a ValueError); ('snr', nsigma[, grow]) is the two-pass form, per band:
    a plain solve, ``mask_from_map`` of its map, and the solve again on the same set-up, which takes
    the per-band loop as ``noise_prior`` does.  Every file written gains a 'SolveMask' image HDU; each
    band's entry gains 'solve_mask'.  Not with ``ground``, ``residual_cut`` or ``healpix``."""
    solve_mask = _mask_spec(solve_mask)
    _mask_check(solve_mask, ground or None, residual_cut, healpix)
    noise_prior = _prior_spec(noise_prior)
    if noise_prior is not None and ground:
        raise NotImplementedError('noise_prior with ground_template is not supported')
    if ground and (residuals or residual_cut is not None):
        raise NotImplementedError('residual_chi2 / residual_cut with ground_template is not supported')
    resid = bool(residuals) or residual_cut is not None
    rkw = dict(residuals=bool(residuals), residual_cut=residual_cut) if resid else {}
    if split is not None and isinstance(split, str):
        split = [split]
    if split and ground:
        raise NotImplementedError('split_maps with ground_template is not supported')
    rank, size = _rank_size()
    if device is None:
        import torch
        device = torch.cuda.current_device()
    input_filelist = np.loadtxt(filelistname, dtype=str, ndmin=1) if isinstance(filelistname, str) \
        else np.asarray(filelistname)
    open_file = COMAPData._opener(store)
    filelist, source = [], None
    for i, f in enumerate(input_filelist):
        h = open_file(f)
        if i == 0:
            source = h.attrs('comap')['source'].split(',')[0]
        if 'averaged_tod/tod' in h:
            filelist.append(f)
    filelist = np.array(filelist)
    if isinstance(crval[0], str):
        crval = [sex2deg(c, hours=hr) for c, hr in zip(crval, [True, False])]
    map_info = COMAPData.map_info_from(crval, cdelt, crpix, ctype, nxpix, nypix)
    filelist = _rank_files(filelist, rank, size, offset_length, feeds, map_info, healpix, open_file)
    if source in CALIBRATORS:
        offset_length = 250
        threshold = 1
    out = {}
    mkw = {}
    if solve_mask is not None:
        mkw = {'solve_mask': solve_mask if _snr_spec(solve_mask) else read_solve_mask(solve_mask, nypix, nxpix)}
    fnoise = None
    if noise_prior == 'fnoise':
        # (a rank's missing dataset fails every rank, before the solves' collectives)
        fnoise, _ = _on_every_rank('noise prior', lambda: fnoise_tables(filelist, open_file, bands))
    if batch_bands and len(bands) > 1 and not ground and noise_prior is None and not _snr_spec(solve_mask):
        r = COMAPData.read_comap_data_bands(filelist, map_info, bands=bands, offset_length=offset_length, feeds=feeds,
                                            use_gain_filter=use_gain_filter, calibration=calibration,
                                            calibrator=calibrator, healpix=healpix, store=store, device=device)
        pixel_edges = _healpix_edges(r['pointing']) if healpix else np.arange(nxpix * nypix)
        res = run_destriper_bands(r['pointing'], r['tod'], r['weights'], offset_length, pixel_edges, keep=r['keep'],
                                  threshold=threshold, niter=niter, device=device,
                                  map_shape=None if healpix else (nypix, nxpix), split=split or None,
                                  feedid=r['feedid'], obsids=r['obsids'], **rkw, **mkw)
        for iband, maps in zip(bands, res):
            sky = {k: v for k, v in maps.items()
                   if k not in ('iters', 'offsets', 'Residuals', 'solve_mask')}    # 'All' and the split maps
            if rank == 0:
                if healpix:
                    write_map_healpix(prefix, sky, r['remapping_array'], map_info, output_dir, iband)
                elif mkw:
                    write_map(prefix, sky, map_info, output_dir, iband, solve_mask=maps['solve_mask']['mask'])
                else:
                    write_map(prefix, sky, map_info, output_dir, iband)
                if resid:
                    _write_residuals(output_dir, prefix, iband, maps['Residuals'])
            if resid:
                sky = dict(sky, Residuals=maps['Residuals'])
            if mkw:
                sky = dict(sky, solve_mask=maps['solve_mask'])
            # (with split maps the band's entry keeps the offsets they were binned with)
            out[iband] = dict(sky, offsets=maps['offsets']) if split else sky       # (on every rank, as per band)
        return out
    for iband in bands:
        tod, weights, pointing, remap, az, el, ra, dec, feedid, obsids = COMAPData.read_comap_data(
            filelist, map_info, feed_weights=feed_weights, offset_length=offset_length, iband=iband, feeds=feeds,
            use_gain_filter=use_gain_filter, calibration=calibration, calibrator=calibrator, healpix=healpix,
            store=store, device=device)
        pixel_edges = _healpix_edges(pointing) if healpix else np.arange(nxpix * nypix)
        prior = None
        if fnoise is not None:
            prior = {'table': fnoise[iband]}
        elif noise_prior is not None:
            prior = dict(zip(('fknee', 'alpha', 'taps'), noise_prior))
        maps = run_destriper(pointing, tod, weights, offset_length, pixel_edges, az, el, ra, dec, feedid, obsids,
                             obsid_cuts, threshold=threshold, niter=niter, chi2_cutoff=20,
                             device=device, map_shape=None if healpix else (nypix, nxpix), ground=ground,
                             split=split or None, prior=prior, **rkw, **mkw)
        sky = {k: v for k, v in maps.items()
               if k not in ('Ground', 'offsets', 'Residuals', 'solve_mask')}    # (the writers iterate the dict: the maps only)
        if rank == 0:
            if healpix:
                write_map_healpix(prefix, sky, remap, map_info, output_dir, iband)
            elif mkw:
                write_map(prefix, sky, map_info, output_dir, iband, solve_mask=maps['solve_mask']['mask'])
            else:
                write_map(prefix, sky, map_info, output_dir, iband)
            if ground:
                os.makedirs(output_dir, exist_ok=True)
                np.savez(os.path.join(output_dir, '{}_ground_band{}.npz'.format(prefix, iband)), **maps['Ground'])
            if resid:
                _write_residuals(output_dir, prefix, iband, maps['Residuals'])
        out[iband] = maps
    return out


def _write_residuals(output_dir, prefix, iband, table):
    os.makedirs(output_dir, exist_ok=True)
    np.savez(os.path.join(output_dir, '{}_residuals_band{}.npz'.format(prefix, iband)), **table)


def residual_params(params):
    """(residuals, residual_cut) from the [Inputs] section: ``residual_chi2`` (True / False) and
    ``residual_cut`` (a number); an absent key, None or False means off."""
    chi2, cut = params.get('residual_chi2'), params.get('residual_cut')
    if isinstance(cut, bool) or cut is None:
        if cut is True:
            raise ValueError('[Inputs] residual_cut must be a number')
        cut = None
    elif not isinstance(cut, float):
        raise ValueError(f'[Inputs] residual_cut must be a number, not {cut!r}')
    if not (chi2 is None or isinstance(chi2, bool)):
        raise ValueError(f'[Inputs] residual_chi2 must be True or False, not {chi2!r}')
    return bool(chi2), cut


def read_solve_mask(fname, nypix, nxpix):
    """The solve mask of a FITS file: its first image HDU, (nypix, nxpix), non-zero = masked, as bool
    [nypix, nxpix].  ValueError for another shape and for a NaN."""
    hdus = read_image_hdus(fname)
    if not hdus:
        raise ValueError(f'solve_mask: {fname} holds no image HDU')
    img = hdus[0][1]
    if img.shape != (int(nypix), int(nxpix)):
        raise ValueError(f'solve_mask: {fname} is {img.shape}, the map ({int(nypix)}, {int(nxpix)})')
    if np.isnan(img).any():
        raise ValueError(f'solve_mask: {fname} holds a NaN')
    return img != 0


def _mask_spec(v):
    """``main``'s solve_mask as None, a file name or ('snr', nsigma, grow); ValueError otherwise."""
    if v is None or v is False:
        return None
    if isinstance(v, str):
        if v == 'snr':
            raise ValueError('solve_mask snr needs <nsigma>: snr, <nsigma>[, <grow>]')
        return v
    if isinstance(v, (tuple, list)) and len(v) in (2, 3) and v[0] == 'snr':
        try:
            nsigma, grow = _snr_spec(tuple(v))
        except (TypeError, ValueError):
            raise ValueError(f'solve_mask must be a FITS file or snr, <nsigma>[, <grow>], not {v!r}') from None
        return ('snr', nsigma, grow)
    raise ValueError(f'solve_mask must be a FITS file or snr, <nsigma>[, <grow>], not {v!r}')


def mask_params(params):
    """``main``'s solve_mask from the [Inputs] section: ``solve_mask : <file.fits>`` or ``solve_mask :
    snr, <nsigma>[, <grow>]``; an absent key, None or False means off.  ValueError for anything else."""
    return _mask_spec(params.get('solve_mask'))


def _prior_spec(v):
    """``main``'s noise_prior as None, 'fnoise' or (fknee, alpha, taps); ValueError otherwise."""
    if v is None or v is False:
        return None
    if isinstance(v, str):
        if v != 'fnoise':
            raise ValueError(f"noise_prior must be 'fnoise' or <fknee>, <alpha>[, <taps>], not {v!r}")
        return v
    try:
        vals = [float(x) for x in v]
    except (TypeError, ValueError):
        raise ValueError(f"noise_prior must be 'fnoise' or <fknee>, <alpha>[, <taps>], not {v!r}") from None
    if len(vals) not in (2, 3):
        raise ValueError(f'noise_prior takes <fknee>, <alpha>[, <taps>], not {len(vals)} values')
    fknee, alpha, taps = vals[0], vals[1], vals[2] if len(vals) == 3 else 16.0
    if not (np.isfinite(fknee) and fknee > 0):
        raise ValueError(f'noise_prior: fknee must be a positive number, not {fknee}')
    if not (np.isfinite(alpha) and alpha < 0):
        raise ValueError(f'noise_prior: alpha must be a negative number, not {alpha}')
    if taps != int(taps) or not 1 <= taps <= 64:
        raise ValueError(f'noise_prior: taps must be a whole number in 1 .. 64, not {taps}')
    return fknee, alpha, int(taps)


def prior_params(params):
    """``main``'s noise_prior from the [Inputs] section: ``noise_prior : fnoise`` or
    ``noise_prior : <fknee>, <alpha>[, <taps>]``; an absent key, None or False means off.
    ValueError for anything else."""
    v = params.get('noise_prior')
    if isinstance(v, bool) and v:
        raise ValueError("[Inputs] noise_prior must be 'fnoise' or <fknee>, <alpha>[, <taps>]")
    if isinstance(v, float):
        raise ValueError('[Inputs] noise_prior takes <fknee>, <alpha>[, <taps>], not 1 value')
    return _prior_spec(v)


def fnoise_tables(filelist, open_file, bands):
    """{band: {(obsid, feed): (fknee, alpha)}} from every file's Level-2 red-noise fits
    ``fnoise_fits/fnoise_fit_parameters`` [feed row, band, scan, (sigma_white, sigma_red, alpha)]:
    per (file, feed, band) the medians of fknee (``fknee_from_red_noise``) and alpha over the scans
    with a valid fit; a (file, feed, band) without one is left out (its group gets no prior).
    ValueError, naming it, for a file without the dataset."""
    name = 'fnoise_fits/fnoise_fit_parameters'
    out = {b: {} for b in bands}
    for fn in filelist:
        f = open_file(fn)
        if name not in f:
            raise ValueError(f'noise_prior fnoise: {fn} has no {name}')
        par = np.asarray(f[name], dtype=np.float64)
        feeds = np.asarray(f['spectrometer/feeds']).astype(np.int64)
        obsid = int(os.path.basename(str(fn)).split('-')[1])
        for row, feed in enumerate(feeds[:par.shape[0]]):
            for b in bands:
                if b >= par.shape[1]:
                    continue
                fits = par[row, b].reshape(-1, 3)
                fknee = np.atleast_1d(fknee_from_red_noise(fits[:, 0], fits[:, 1], fits[:, 2]))
                ok = np.isfinite(fknee)
                if ok.any():
                    out[b][obsid, int(feed)] = (float(np.median(fknee[ok])), float(np.median(fits[ok, 2])))
    return out


def cli(argv):
    """``__main__`` block of run_destriper.py (:191-212): everything from [Inputs]
    except use_gain_filter / calibration / calibrator from [ReadData]."""
    p = Parser(argv[0])
    params = p['Inputs']
    feeds = params['feeds']
    feeds = [int(f) for f in (feeds if isinstance(feeds, list) else [feeds])]
    as_list = lambda v: v if isinstance(v, list) else [v]  # noqa: E731
    split = params.get('split_maps')             # 'feed', 'obsid' or both (a list); absent or None: no split maps
    residuals, residual_cut = residual_params(params)
    return main(params['filelistname'], offset_length=int(params['offset_length']), prefix=params['prefix'],
                output_dir=params['output_dir'], feeds=feeds, feed_weights=params['feed_weights'],
                nxpix=int(params['nxpix']), nypix=int(params['nypix']), crval=as_list(params['crval']),
                crpix=as_list(params['crpix']), ctype=as_list(params['ctype']), cdelt=as_list(params['cdelt']),
                use_gain_filter=p['ReadData']['use_gain_filter'], calibration=p['ReadData']['calibration'],
                calibrator=p['ReadData']['calibrator'], threshold=10 ** float(params['threshold']),
                niter=int(params['niter']), healpix=params['healpix'],
                ground=bool(params.get('ground_template', False)),
                split=[str(k) for k in as_list(split)] if split else None, residuals=residuals,
                residual_cut=residual_cut, noise_prior=prior_params(params), solve_mask=mask_params(params))
