"""Cost of the destriper's noise prior: the CG on (A + T) against the plain solve.

    python scripts/ds_prior.py [--obs 8] [--taps 16 64] [--rounds 3] [--plain-only] [--kernel-only]
                               [--label NAME] [--out FILE]

Inputs: synthetic.level2_mapmaking observations (19 feeds, 45 000 samples) through
COMAPData.read_comap_data_bands (band 0, L = 50) onto the 480 x 480 CAR map, on the tiled layout; 8
observations are the C5 share of one GPU, one band.  Per configuration (plain, prior with each
``taps``), over ``rounds`` (median and range reported):

* ms per CG iteration -- two native solves with the stop test off (threshold 0), of N1 = 32 and
  N2 = 160 iterations, a host clock around each ending in a device synchronise; the difference over
  N2 - N1 (set-up of the solve, the final maps and the read-backs cancel);
* iterations to 1e-6.

The prior is the driver's one-model form: fknee 0.2 Hz, alpha -1.5, groups per (observation, feed),
each stencil scaled by the group's largest weight.  --plain-only touches nothing the prior added, so
the same script times the parent commit's plain solve on the same box (--label parent).  With
--kernel-only, nothing but two warmed prior solves per ``taps``, for a rocprofv3 --kernel-trace
--stats run of its own.  Prints one JSON line per configuration."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

N1, N2 = 32, 160
FKNEE, ALPHA = 0.2, -1.5


def inputs(n_obs, device, first=21):
    from comapreduce_amd import synthetic
    from comapreduce_amd.mapmaking import comapdata as CD
    store = {}
    for o in range(n_obs):
        data, attrs, fn = synthetic.level2_mapmaking(first + o)
        store[fn] = (data, attrs)
    mi = CD.map_info_from([synthetic.FIELD_RA, synthetic.FIELD_DEC], [-1.0 / 60.0, 1.0 / 60.0], [240, 240],
                          ['RA---CAR', 'DEC--CAR'], 480, 480)
    return CD.read_comap_data_bands(list(store), mi, bands=(0,), offset_length=50, store=store, device=device)


def timed(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def per_iteration(solve, rounds):
    """(ms per iteration over the rounds, iterations to 1e-6) of solve(threshold, niter)."""
    solve(0.0, N1), solve(0.0, N2)                       # warm: code objects, vectors, the graph
    ms = []
    for _ in range(rounds):
        (_, it1, _), t1 = timed(lambda: solve(0.0, N1))
        (_, it2, _), t2 = timed(lambda: solve(0.0, N2))
        assert it1[0] == N1 and it2[0] == N2, (it1, it2)
        ms.append((t2 - t1) / (N2 - N1))
    _, it, _ = solve(1e-6, 400)
    return ms, int(it[0])


def measure(n_obs, taps, rounds, device, plain_only, kernel_only, label):
    import torch
    from comapreduce_amd.mapmaking import destriper as D
    assert torch.cuda.is_available(), 'ds_prior.py measures on the GPU only'
    L, npix = 50, 480 * 480
    r = inputs(n_obs, device)
    pix = np.asarray(r['pointing']).astype(np.int32)
    tod, w = np.asarray(r['tod'])[0], np.asarray(r['weights'])[0]
    out = []

    def line(name, ms, it, dd, **extra):
        nnz = dd.ops.nnz()
        out.append({'label': label, 'configuration': name, 'observations': n_obs, 'n_offsets': dd.ops.n_offsets,
                    'nnz': list(nnz), 'ms_per_iteration': statistics.median(ms), 'ms_range': [min(ms), max(ms)],
                    'ms_all': ms, 'iterations_to_1e-6': it, **extra})
        print(json.dumps(out[-1]), flush=True)

    if not kernel_only:
        dd = D.DeviceDestriper(pix, tod, w, L, npix, device, map_shape=(480, 480))
        ms, it = per_iteration(dd.ops.solve_native, rounds)
        line('plain', ms, it, dd)
        del dd
    if plain_only:
        return out
    for K in taps:
        model = {'fknee': FKNEE, 'alpha': ALPHA, 'taps': K, 'feedid': r['feedid'], 'obsids': r['obsids']}
        dd = D.DeviceDestriper(pix, tod, w, L, npix, device, map_shape=(480, 480), prior=model)
        groups = int((dd.pops.gid >= 0).sum().item())
        if kernel_only:
            for _ in range(2):
                dd.pops.solve_native(0.0, N1)
            torch.cuda.synchronize()
            out.append({'label': label, 'configuration': f'prior taps {K}', 'kernel_only_iterations': 2 * N1})
            print(json.dumps(out[-1]), flush=True)
        else:
            ms, it = per_iteration(dd.pops.solve_native, rounds)
            line(f'prior taps {K}', ms, it, dd, taps=K, offsets_with_prior=groups)
        del dd
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--obs', type=int, default=8)
    ap.add_argument('--taps', type=int, nargs='+', default=[16, 64])
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--plain-only', action='store_true', help='the plain solve only (runs on the parent commit too)')
    ap.add_argument('--kernel-only', action='store_true', help='warmed prior solves only (for a kernel trace)')
    ap.add_argument('--label', default='new')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import torch
    lines = measure(a.obs, a.taps, a.rounds, torch.cuda.current_device(), a.plain_only, a.kernel_only, a.label)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'a') as f:
            f.write(''.join(json.dumps(v) + '\n' for v in lines))


if __name__ == '__main__':
    main()
