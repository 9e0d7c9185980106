"""Cost of the destriper's residual chi-squared pass: the device pass
(comap_destripe_residuals: per offset, then per (observation, feed) group) against the only route
there was before it, the same statistics written with torch ops on the device.

    python scripts/ds_resid.py [--obs 1 8] [--bands 1 4] [--rounds 3] [--kernel-only] [--out FILE]

Inputs: synthetic.level2_mapmaking observations (19 feeds, 45 000 samples) through
COMAPData.read_comap_data_bands (L = 50) onto the 480 x 480 CAR map, on the tiled layout; 1
observation is the C4 problem, 8 the C5 share of one GPU.  Per size and band count, a host clock
around work that ends in a device synchronise, the routes alternated over ``rounds`` (median and
range reported):

* native -- DeviceOps.residuals on the solved device offsets and map: the per-offset pass, the
            group sort and sums, the one read-back;
* torch  -- a gather of the map per sample, the residual and its term as tensor expressions,
            index_add_ per offset, then index_add_ per group (sums in whatever order the atomics
            land: close to the native sums, not equal; the counts are equal).

Also the pass's algorithmic bytes -- N (4 + 16 nb) of pix, tod and w, plus x, the outputs and the
map gather (8 nb per binned sample) -- and the share of the HBM rates (8.0 TB/s specified, 6.3 TB/s
as a streaming copy reaches) that the native time corresponds to.  With --kernel-only, nothing but
warmed native calls, for a rocprofv3 --kernel-trace --stats run of its own.  Prints one JSON line
per configuration."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_SPEC, HBM_COPY = 8.0e12, 6.3e12          # bytes / s


def inputs(n_obs, bands, device, first=21):
    from comapreduce_amd import synthetic
    from comapreduce_amd.mapmaking import comapdata as CD
    store = {}
    for o in range(n_obs):
        data, attrs, fn = synthetic.level2_mapmaking(first + o)
        store[fn] = (data, attrs)
    mi = CD.map_info_from([synthetic.FIELD_RA, synthetic.FIELD_DEC], [-1.0 / 60.0, 1.0 / 60.0], [240, 240],
                          ['RA---CAR', 'DEC--CAR'], 480, 480)
    return CD.read_comap_data_bands(list(store), mi, bands=bands, offset_length=50, store=store, device=device)


def timed(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def measure(n_obs, n_bands, rounds, device, kernel_only=False):
    import torch
    from comapreduce_amd.mapmaking import destriper as D
    assert torch.cuda.is_available(), 'ds_resid.py measures on the GPU only'
    L, npix = 50, 480 * 480
    r = inputs(n_obs, tuple(range(n_bands)), device)
    pix = np.asarray(r['pointing']).astype(np.int32)
    tod, w, keep = (np.asarray(r[k]) for k in ('tod', 'weights', 'keep'))
    if n_bands == 1:
        tod, w = tod[0], w[0]
    gid, uobs, ufeed = D.ground_groups(r['feedid'], r['obsids'], L)
    G = int(uobs.size * ufeed.size)
    dd = D.DeviceDestriper(pix, tod, w, L, npix, device, keep=keep, map_shape=(480, 480), residuals=(gid, G))
    ops = dd.ops
    xs, _, maps = ops.solve_native(1e-6, 100)        # x in the caller's order, the map in the internal layout
    m = maps['map']
    gid_d = dd.resid[0]
    nb, NO, N = ops.nb, ops.n_offsets, int(pix.size)

    def native():
        return ops.residuals(xs, m, gid_d, G)

    if kernel_only:
        for _ in range(3):
            native()
        torch.cuda.synchronize()
        return {'observations': n_obs, 'bands': n_bands, 'groups': G, 'kernel_only_calls': 3}

    pix_l = ops.pix.to(torch.int64)
    binned = pix_l >= 0
    off = torch.arange(N, device=ops.dev) // L
    g64 = gid_d.to(torch.int64)
    in_group = g64 >= 0

    def by_torch():
        mg = m.view(-1, nb)[pix_l.clamp(min=0)].t()                          # [nb, N]: the gather of the map
        xr = xs.view(NO, nb).t().repeat_interleave(L, dim=1)
        res = (ops.tod - xr) - mg
        counted = binned[None, :] & (ops.w > 0)
        if ops.keep is not None:
            counted &= ops.keep.repeat_interleave(L, dim=1) != 0
        term = torch.where(counted, (ops.w * res) * res, torch.zeros_like(res))
        off_sum = torch.zeros((nb, NO), dtype=torch.float64, device=ops.dev).index_add_(1, off, term)
        off_cnt = torch.zeros((nb, NO), dtype=torch.int64, device=ops.dev).index_add_(1, off, counted.to(torch.int64))
        grp_sum = torch.zeros((nb, G), dtype=torch.float64, device=ops.dev).index_add_(1, g64[in_group], off_sum[:, in_group])
        grp_cnt = torch.zeros((nb, G), dtype=torch.int64, device=ops.dev).index_add_(1, g64[in_group], off_cnt[:, in_group])
        return off_sum, off_cnt, grp_sum, grp_cnt

    routes = {'native': native, 'torch': by_torch}
    for fn in routes.values():               # warm every path (code objects, allocations)
        fn()
    ms = {k: [] for k in routes}
    for _ in range(rounds):
        for k, fn in routes.items():
            ms[k].append(timed(fn)[1])
    a, b = native(), by_torch()
    cnt_equal = bool(torch.equal(a[1].view(NO, nb).t().to(torch.int64), b[1])
                     and torch.equal(a[3].view(G, nb).t(), b[3]))
    gs, gt = a[2].view(G, nb).t(), b[2]
    rel = float(((gs - gt).abs() / gt.abs().clamp(min=1e-300)).max().item())
    med = {k: statistics.median(v) for k, v in ms.items()}
    n_binned = int(binned.sum().item())
    nbytes = N * (4 + 16 * nb) + 8 * nb * n_binned + NO * nb * (8 + 8 + 4) + (NO * nb if ops.keep is not None else 0) \
        + NO * 4 + G * nb * 16
    rate = nbytes / (med['native'] * 1e-3)
    return {'observations': n_obs, 'bands': n_bands, 'bands_run': nb, 'groups': G, 'n_samples': N, 'n_offsets': NO,
            'ms': med, 'ms_range': {k: [min(v), max(v)] for k, v in ms.items()}, 'ms_all': ms,
            'torch_over_native': med['torch'] / med['native'], 'algorithmic_bytes': nbytes,
            'native_bytes_per_s': rate, 'share_of_hbm_spec': rate / HBM_SPEC, 'share_of_hbm_copy': rate / HBM_COPY,
            'counts_equal': cnt_equal, 'group_sum_relmax_torch_vs_native': rel}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--obs', type=int, nargs='*', default=[1, 8])
    ap.add_argument('--bands', type=int, nargs='+', default=[1, 4])
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--kernel-only', action='store_true', help='warmed native calls only (for a kernel trace)')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import torch
    device = torch.cuda.current_device()
    lines = []
    for n in a.obs:
        for nb in a.bands:
            lines.append(json.dumps(measure(n, nb, a.rounds, device, a.kernel_only)))
            print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
