"""Cost of the destriper's split maps: the one-pass device route
(comap_destripe_split_maps for all labels, then the division) against the only route there was
before it, one DeviceOps set-up per label just for its local_maps().

    python scripts/ds_split.py [--obs 1 8] [--bands 1 4] [--by feed obsid] [--pile 1000 100000] [--rounds 3] [--out FILE]

Inputs: synthetic.level2_mapmaking observations (19 feeds, 45 000 samples) through
COMAPData.read_comap_data_bands (L = 50) onto the 480 x 480 CAR map, on the tiled layout; 1
observation is the C4 problem, 8 the C5 share of one GPU.  Per size, band count and split kind, a
host clock around work that ends in a device synchronise, the routes alternated over ``rounds``
(median and range reported):

* one_pass  -- DeviceDestriper._split_maps on the solved device offsets: the sort, the sums, the
               division and the layout back to the caller's pixel order, every label at once;
* per_label -- for each label g: ONE DeviceOps(pix[sel], (tod - repeat(x, L))[sel], w[sel], ...)
               .local_maps() (the operator is never used): numerator, weight and hits, undivided, and
               no naive map; device-side selection included, as a caller would have to do it;
* per_label_naive -- per_label plus a second DeviceOps on tod[sel] per label for the naive numerator,
               and the division: everything the one pass returns;
* solve     -- the set-up plus the solve of the same problem (threshold 1e-6, 100 iterations at
               most), which the split pass is reported as a share of.

Also the longest (label, pixel) row of each labelling -- a serial chain in the summing kernel by
the definition of the order -- and, with --kernel-only, nothing but warmed one-pass calls, for a
rocprofv3 --kernel-trace --stats run of its own.  ``--pile R ...``: the C call alone on 1e6 synthetic
samples of which R fall in one (label, pixel) row, the field-scale heavy row that the synthetic
observations lack.  Prints one JSON line per configuration."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


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


def longest_row(pix, labels, L, npix):
    """(samples in the fullest (label, pixel) row, samples in the fullest pixel over all labels)."""
    pix = np.asarray(pix, np.int64)
    lab = np.repeat(np.asarray(labels, np.int64), L)
    ok = (pix >= 0) & (lab >= 0)
    per_row = np.bincount(lab[ok] * npix + pix[ok])
    return int(per_row.max()), int(np.bincount(pix[ok]).max())


def measure(n_obs, n_bands, by, rounds, device, kernel_only=False):
    import torch
    from comapreduce_amd.mapmaking import destriper as D
    assert torch.cuda.is_available(), 'ds_split.py measures on the GPU only'
    L, npix = 50, 480 * 480
    r = inputs(n_obs, tuple(range(n_bands)), device)
    pix = np.asarray(r['pointing']).astype(np.int32)
    tod, w, keep = (np.asarray(r[k]) for k in ('tod', 'weights', 'keep'))
    if n_bands == 1:
        tod, w = tod[0], w[0]
    labels, names = D.split_labels(by, r['feedid'], r['obsids'], L)
    G = len(names)

    def build():
        return D.DeviceDestriper(pix, tod, w, L, npix, device, keep=keep, map_shape=(480, 480), split=(labels, G))

    def solve():
        dd = build()
        dd.split = None                      # the plain set-up and solve, without the split pass
        return dd.solve(1e-6, 100)['iters']

    dd = build()
    ops = dd.ops
    xs = ops.solve_native(1e-6, 100)[0]      # [N/L * nb], the caller's order

    def one_pass():
        return dd._split_maps(xs)

    if kernel_only:
        for _ in range(3):
            one_pass()
        torch.cuda.synchronize()
        return {'observations': n_obs, 'bands': n_bands, 'by': by, 'labels': G, 'kernel_only_calls': 3}

    # the per-label route on the same device arrays (row-major pixels: each label's own operator)
    pix_d = torch.from_numpy(pix).to(ops.dev)
    lab_s = torch.from_numpy(np.repeat(labels, L)).to(ops.dev)
    tod_d, w_d = ops.tod[:ops.n_bands], ops.w[:ops.n_bands]
    x_d = xs.reshape(-1, ops.nb).t()[:ops.n_bands].repeat_interleave(L, dim=1)
    keep_d = None if ops.keep is None else ops.keep[:ops.n_bands].repeat_interleave(L, dim=1)

    def per_label(naive=False):
        out = []
        z = tod_d - x_d                      # tod - F x, once for all labels
        for g in range(G):
            sel = torch.nonzero(lab_s == g).reshape(-1)
            kp = None if keep_d is None else keep_d[:, sel][:, ::L].contiguous()
            a = D.DeviceOps(pix_d[sel], z[:, sel], w_d[:, sel], L, npix, device, keep=kp)
            h, hits, num = a.local_maps()
            if naive:
                b = D.DeviceOps(pix_d[sel], tod_d[:, sel], w_d[:, sel], L, npix, device, keep=kp)
                nn = b.local_maps()[2]
                m, nv = ops.split_div(num, nn, h)
                out.append((m, nv, h, hits))
            else:
                out.append((num, None, h, hits))
        return out

    routes = {'one_pass': one_pass, 'per_label': per_label, 'per_label_naive': lambda: per_label(True),
              'solve': solve}
    for fn in routes.values():               # warm every path (code objects, allocations, the graph)
        fn()
    ms = {k: [] for k in routes}
    for _ in range(rounds):
        for k, fn in routes.items():
            ms[k].append(timed(fn)[1])
    # both routes bin the same samples: the weight maps must agree bit for bit
    sp, ref = one_pass(), per_label()
    wt = sp['weight'] if n_bands > 1 else sp['weight'][None]
    same = all(torch.equal(wt[:, g].reshape(-1), ref[g][2].reshape(npix, -1).t()[:wt.shape[0]].reshape(-1))
               for g in range(G))
    med = {k: statistics.median(v) for k, v in ms.items()}
    row, pixel = longest_row(pix, labels, L, npix)
    return {'observations': n_obs, 'bands': n_bands, 'by': by, 'labels': G, 'n_samples': int(pix.size),
            'n_offsets': ops.n_offsets, 'ms': med, 'ms_range': {k: [min(v), max(v)] for k, v in ms.items()},
            'ms_all': ms, 'per_label_over_one_pass': med['per_label'] / med['one_pass'],
            'per_label_naive_over_one_pass': med['per_label_naive'] / med['one_pass'],
            'one_pass_share_of_setup_plus_solve': med['one_pass'] / med['solve'],
            'longest_label_pixel_row': row, 'fullest_pixel_all_labels': pixel, 'weight_maps_equal': bool(same)}


def measure_pile(row, rounds, n=1_000_000, L=50, npix=480 * 480):
    """The serial heavy row at field scale, which the synthetic observations do not have: n samples
    spread over the map, of which ``row`` (whole offsets of label 0) fall in ONE pixel, through the C
    call alone (one band, two labels alternating by offset)."""
    import torch
    from comapreduce_amd import _native as N
    rng = np.random.default_rng(row)
    labels = (np.arange(n // L) % 2).astype(np.int32)
    pix = rng.integers(0, npix, n).astype(np.int32).reshape(-1, L)
    pix[np.nonzero(labels == 0)[0][:row // L]] = npix // 2 + 7
    dev = torch.device('cuda', N.current_device())
    c = N.ctx()
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(device=dev, dtype=dt)  # noqa: E731
    pix_d, lab_d = t(pix.reshape(-1), torch.int32), t(labels, torch.int32)
    tod, w, x = t(rng.standard_normal(n), torch.float64), t(0.5 + rng.random(n), torch.float64), \
        t(rng.standard_normal(n // L), torch.float64)
    out = [N.device_empty(2 * npix, torch.float64, dev) for _ in range(4)]

    def call():
        N.bind_stream(c, dev)
        N.check(N.lib().comap_destripe_split_maps(c, N.dptr(pix_d), N.dptr(tod), N.dptr(w), None, N.dptr(x), N.dptr(lab_d),
                                                  2, n, L, npix, 1, *(N.dptr(o) for o in out)), c, 'split_maps')
    call()
    ms = [timed(call)[1] for _ in range(rounds)]
    got = float(out[3].reshape(2, npix)[0, npix // 2 + 7].item())
    return {'pile_up_row': row, 'n_samples': n, 'hits_in_row': got, 'ms': statistics.median(ms),
            'ms_range': [min(ms), max(ms)]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--obs', type=int, nargs='*', default=[1, 8])
    ap.add_argument('--bands', type=int, nargs='+', default=[1, 4])
    ap.add_argument('--by', nargs='+', default=['feed', 'obsid'])
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--kernel-only', action='store_true', help='warmed one-pass calls only (for a kernel trace)')
    ap.add_argument('--out', default=None)
    ap.add_argument('--pile', type=int, nargs='*', default=[], help='also: the C call with a row of this many samples')
    a = ap.parse_args()
    import torch
    device = torch.cuda.current_device()
    lines = []
    for row in a.pile:
        lines.append(json.dumps(measure_pile(row, a.rounds)))
        print(lines[-1], flush=True)
    for n in a.obs:
        for nb in a.bands:
            for by in a.by:
                lines.append(json.dumps(measure(n, nb, by, a.rounds, device, a.kernel_only)))
                print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
