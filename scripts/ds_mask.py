"""Cost of the destriper's solve mask: building the view against a second full
set-up on the masked weights, and the CG on the view against the plain solve.

    python scripts/ds_mask.py [--obs 8] [--bands 1 4] [--fractions 0.01 0.10] [--rounds 3] [--plain-only]
                              [--kernel-only] [--label NAME] [--out FILE]

Inputs: synthetic.level2_mapmaking observations (19 feeds, 45 000 samples) through
COMAPData.read_comap_data_bands (L = 50) onto the 480 x 480 CAR map, on the tiled layout; 8
observations are the C5 share of one GPU.  The mask holds the given fraction of the hit pixels, those
nearest the map's centre (one compact region, as a source mask is).  Per band count and fraction,
over ``rounds`` (median and range reported):

* view build: DeviceOps.masked_view (comap_destripe_mask_view) on the mask already on the device, a
  host clock around the call ending in a device synchronise; against the bytes it should stream --
  read (4 + c)(nnz + nsell) + c nnzp, written c (nnz + nsell + nnzp), c = NB (count form) or 8 NB
  bytes of coefficients per entry, plus the touched offsets' samples, the offset sums and the maps;
* full set-up on w': DeviceOps (comap_destripe_create_keyed, the same offset keys) on the masked
  weights, which is what a caller had to do without the view;
* ms per CG iteration, plain and masked -- two native solves with the stop test off (threshold 0), of
  N1 = 32 and N2 = 160 iterations; the difference over N2 - N1;
* iterations to 1e-6.

--plain-only touches nothing the mask added, so the same script times the parent commit's plain solve
on the same box (--label parent).  With --kernel-only, nothing but one view build and two warmed
masked solves per configuration, for a rocprofv3 --kernel-trace --stats run of its own.  Prints one
JSON line per configuration."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

N1, N2 = 32, 160
NY = NX = 480


def inputs(n_obs, bands, device, first=21):
    from comapreduce_amd import synthetic
    from comapreduce_amd.mapmaking import comapdata as CD
    store = {}
    for o in range(n_obs):
        data, attrs, fn = synthetic.level2_mapmaking(first + o)
        store[fn] = (data, attrs)
    mi = CD.map_info_from([synthetic.FIELD_RA, synthetic.FIELD_DEC], [-1.0 / 60.0, 1.0 / 60.0], [240, 240],
                          ['RA---CAR', 'DEC--CAR'], NX, NY)
    return CD.read_comap_data_bands(list(store), mi, bands=bands, offset_length=50, store=store, device=device)


def timed(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def per_iteration(solve, rounds):
    """(ms per iteration over the rounds, iterations to 1e-6 per band) of solve(threshold, niter)."""
    solve(0.0, N1), solve(0.0, N2)                       # warm: code objects, vectors, the graph
    ms = []
    for _ in range(rounds):
        (_, it1, _), t1 = timed(lambda: solve(0.0, N1))
        (_, it2, _), t2 = timed(lambda: solve(0.0, N2))
        assert it1[0] == N1 and it2[0] == N2, (it1, it2)
        ms.append((t2 - t1) / (N2 - N1))
    _, it, _ = solve(1e-6, 400)
    return ms, [int(v) for v in it]


def central_mask(pix, fraction):
    """bool [NY * NX]: the given fraction of the hit pixels, nearest the map's centre first."""
    hit = np.bincount(pix[pix >= 0], minlength=NY * NX) > 0
    y, x = np.divmod(np.nonzero(hit)[0], NX)
    order = np.argsort((y - NY / 2) ** 2 + (x - NX / 2) ** 2, kind='stable')
    mask = np.zeros(NY * NX, bool)
    mask[np.nonzero(hit)[0][order[:max(1, int(round(fraction * hit.sum())))]]] = True
    return mask, int(hit.sum())


def stat(v):
    return {'median': statistics.median(v), 'range': [min(v), max(v)], 'all': v}


def measure(n_obs, nbands, fractions, rounds, device, plain_only, kernel_only, label):
    import torch
    from comapreduce_amd import _native as N
    from comapreduce_amd.mapmaking import destriper as D
    assert torch.cuda.is_available(), 'ds_mask.py measures on the GPU only'
    L, npix = 50, NY * NX
    r = inputs(n_obs, tuple(range(nbands)), device)
    pix = np.asarray(r['pointing']).astype(np.int32)
    tod, w = np.asarray(r['tod']), np.asarray(r['weights'])
    if nbands == 1:
        tod, w = tod[0], w[0]
    out = []

    def line(name, **extra):
        out.append({'label': label, 'configuration': name, 'observations': n_obs, 'bands': nbands, **extra})
        print(json.dumps(out[-1]), flush=True)

    dd = D.DeviceDestriper(pix, tod, w, L, npix, device, map_shape=(NY, NX))
    ops = dd.ops
    nnz, nnzp = ops.nnz()
    nsell = max(ops.sell_entries(), 0)
    if not kernel_only:
        ms, it = per_iteration(ops.solve_native, rounds)
        line('plain', n_offsets=ops.n_offsets, nnz=[nnz, nnzp], sell_entries=nsell, entry_bytes=ops.entry_bytes(),
             ms_per_iteration=stat(ms), iterations_to_1e_6=it)
    if plain_only:
        return out
    cb = ops.entry_bytes() - 4
    for fraction in fractions:
        mask, n_hit = central_mask(pix, fraction)
        name = f'mask {fraction:g}'
        dd.set_solve_mask(mask)
        m = dd.sops.mask
        on = (ops.pix >= 0) & (m[ops.pix.clamp(min=0).to(torch.int64)] != 0)
        touched = int(on.reshape(ops.n_offsets, L).any(dim=1).sum().item())
        if kernel_only:
            for _ in range(2):
                dd.sops.solve_native(0.0, N1)
            torch.cuda.synchronize()
            line(name, kernel_only_iterations=2 * N1, view_builds=1)
            continue
        build = []
        for _ in range(rounds + 1):                      # (the first warms the code objects and the pool)
            view, t = timed(lambda: ops.masked_view(m))
            build.append(t)
            del view
        wm = torch.where(on[None, :], torch.zeros_like(ops.w), ops.w)
        full = []
        for _ in range(rounds + 1):
            other, t = timed(lambda: D.DeviceOps(ops.pix, ops.tod[:ops.n_bands], wm[:ops.n_bands], L, ops.npix, device,
                                                 None if ops.keep is None else ops.keep[:ops.n_bands], dd.okey))
            full.append(t)
            del other
        N.trim_caches()
        nb = ops.nb
        model = ((4 + cb) * (nnz + nsell) + cb * nnzp + cb * (nnz + nsell + nnzp) + touched * L * (4 + 16 * nb)
                 + 4 * 8 * nb * ops.n_offsets + (1 + 4 * 8 * nb) * ops.npix + 8 * ops.n_offsets)
        ms, it = per_iteration(dd.sops.solve_native, rounds)
        info = dd.mask_info
        line(name, hit_pixels=n_hit, masked_pixels=info['pixels'], masked_samples=np.asarray(info['samples']).tolist(),
             empty_offsets=np.asarray(info['empty_offsets']).tolist(), touched_offsets=touched,
             view_build_ms=stat(build[1:]), full_setup_ms=stat(full[1:]), view_model_bytes=model,
             view_gb_per_s=model / (statistics.median(build[1:]) * 1e-3) / 1e9, ms_per_iteration=stat(ms),
             iterations_to_1e_6=it)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--obs', type=int, default=8)
    ap.add_argument('--bands', type=int, nargs='+', default=[1, 4])
    ap.add_argument('--fractions', type=float, nargs='+', default=[0.01, 0.10])
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--plain-only', action='store_true', help='the plain solve only (runs on the parent commit too)')
    ap.add_argument('--kernel-only', action='store_true', help='a view build and warmed masked solves only')
    ap.add_argument('--label', default='new')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import torch
    lines = []
    for nbands in a.bands:
        lines += measure(a.obs, nbands, a.fractions, a.rounds, torch.cuda.current_device(), a.plain_only,
                         a.kernel_only, a.label)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'a') as f:
            f.write(''.join(json.dumps(v) + '\n' for v in lines))


if __name__ == '__main__':
    main()
