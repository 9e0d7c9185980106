"""Cost of the destriper's ground (azimuth) template per CG iteration.

    python scripts/ds_ground.py [--obs 1 8] [--niter 100] [--rounds 3] [--out FILE]
    python scripts/ds_ground.py --ranks 2 [--backends gloo nccl] [--obs 1 4] ...   (ranks mode, below)

C4 inputs: synthetic.level2_mapmaking observations (19 feeds, 45 000 samples) through
COMAPData.read_comap_data (band 0, L = 50) onto the 480 x 480 CAR map, on the tiled layout.
Per problem size, with early exit disabled (threshold 0) and a host clock around work that
ends in a device synchronise, the four drivers alternated over ``rounds`` (median reported):

* ground_native -- comap_destripe_ground_solve (replayed graph batches), the ground default;
* ground   -- cg_solve on GroundOps (offsets + slope and level per (observation, feed));
* eager    -- cg_solve on the plain DeviceOps (the same Python driver, no ground terms);
* native   -- comap_destripe_solve (replayed graph batches), the plain production path.

The two new kernels in isolation: ``calls`` back-to-back launches of comap_destripe_ground_bin
and of comap_destripe_ground_project between device events (launch gaps included; operands
cache-warm), and their rate on the entries they stream, 12 B each (4 B index + 8 B value):
nnz_b entries for the bin, nnz_g for the projection, 2 nnz_g x 12 B for both together (an
upper bound of the bytes, as nnz_b <= nnz_g).  Prints one JSON line per problem size.

Ranks mode (``--ranks R``): R processes on ONE GPU, each with ``--obs`` observations of its own,
joined over each of ``--backends`` in turn (a backend that does not come up on a shared device is
reported as such, not measured).  The sharded ground solve's two drivers on the same ranks,
alternated over ``rounds`` with early exit off, a barrier and a host clock around each solve that
ends in a device synchronise (median reported, every rank's rounds kept):

* ground_batched -- cg_solve_batched on GroundOps (comap_destripe_ground_dist_*: 4 native calls and
  3 all-reduces per iteration, one host read of the flags per 16);
* ground_eager   -- cg_solve on GroundOps with the same all-reduces (11 calls, 3 all-reduces and
  a blocking read of r.r per iteration).

Ranks that share a GPU measure the drivers' host-call cost, not a link: the kernels of the ranks
serialise on the one device and the collective never leaves the host (gloo) or the device."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def c4_inputs(n_obs, device, first=21):
    from comapreduce_amd import synthetic
    from comapreduce_amd.mapmaking import comapdata as CD
    store = {}
    for o in range(n_obs):
        data, attrs, fn = synthetic.level2_mapmaking(first + o)
        store[fn] = (data, attrs)
    mi = CD.map_info_from([synthetic.FIELD_RA, synthetic.FIELD_DEC], [-1.0 / 60.0, 1.0 / 60.0], [240, 240],
                          ['RA---CAR', 'DEC--CAR'], 480, 480)
    tod, w, pix, _, az, _, _, _, feedid, obsids = CD.read_comap_data(list(store), mi, iband=0, offset_length=50,
                                                                     store=store, device=device)
    return tod, w, pix.astype(np.int32), az, feedid, obsids


def timed(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def kernel_ms(fn, calls):
    import torch
    for _ in range(5):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def measure(n_obs, niter, rounds, calls, device):
    import torch
    from comapreduce_amd import _native as N
    from comapreduce_amd.mapmaking import destriper as D
    assert torch.cuda.is_available(), 'ds_ground.py measures on the GPU only'
    tod, w, pix, az, feedid, obsids = c4_inputs(n_obs, device)
    dd = D.DeviceDestriper(pix, tod, w, 50, 480 * 480, device, map_shape=(480, 480), ground=(az, feedid, obsids))
    ops, g = dd.ops, dd.gops
    same = lambda t: t  # noqa: E731
    drivers = {'ground_native': lambda: g.solve_native(0.0, niter)[1],
               'ground': lambda: D.cg_solve(g, same, 0.0, niter)[1],
               'eager': lambda: D.cg_solve(ops, same, 0.0, niter)[1],
               'native': lambda: ops.solve_native(0.0, niter)[1][0]}
    for fn in drivers.values():                 # warm every path (code objects, allocations, the graph)
        fn()
    ms = {k: [] for k in drivers}
    for _ in range(rounds):
        for k, fn in drivers.items():
            it, dt = timed(fn)
            assert it == niter, (k, it)
            ms[k].append(dt / niter * 1e3)
    nnz_g, nnz_b = g.nnz()
    # the two kernels alone, on a CG-like state
    u = torch.randn(g.n_offsets, dtype=torch.float64, device=g.dev)
    h, _, _ = g.local_maps()
    num, y = g.zeros(g.npix), g.zeros(g.n_offsets)
    g.bin(u, 0, num)
    g.project(u, num, h, y)
    _, s, _ = g.split(u)
    lib = N.lib()
    N.bind_stream(g.ctx, g.dev)
    t_bin = kernel_ms(lambda: lib.comap_destripe_ground_bin(g.g, N.dptr(s), N.dptr(num)), calls)
    t_proj = kernel_ms(lambda: lib.comap_destripe_ground_project(g.g, N.dptr(g.xp), N.dptr(s), N.dptr(num), N.dptr(h),
                                                                 N.dptr(y), N.dptr(y[g.NO:])), calls)
    med = {k: statistics.median(v) for k, v in ms.items()}
    return {'observations': n_obs, 'n_samples': int(tod.size), 'n_offsets': ops.n_offsets, 'groups': g.K,
            'niter': niter, 'nnz_offset_pixel': ops.nnz(), 'nnz_ground': [nnz_g, nnz_b],
            'ms_per_iter': med, 'ms_per_iter_all': ms, 'ground_over_eager': med['ground'] / med['eager'],
            'ground_native_over_ground': med['ground_native'] / med['ground'],
            'ground_native_over_native': med['ground_native'] / med['native'],
            'ground_bin_ms': t_bin, 'ground_project_ms': t_proj,
            'ground_bin_GBps': nnz_b * 12 / t_bin / 1e6, 'ground_project_GBps': nnz_g * 12 / t_proj / 1e6,
            'both_GBps_on_2nnz12': 2 * nnz_g * 12 / (t_bin + t_proj) / 1e6}


def _ranks_worker(rank, world, port, backend, obs, niter, rounds, q):
    """One rank of the ranks mode: per problem size, both drivers alternated; rank 0 reports."""
    try:
        import torch
        import torch.distributed as dist
        from comapreduce_amd.mapmaking import destriper as D
        os.environ['MASTER_ADDR'] = '127.0.0.1'
        os.environ['MASTER_PORT'] = str(port)
        torch.cuda.set_device(0)
        dist.init_process_group(backend, rank=rank, world_size=world)
        out = []
        for n_obs in obs:
            tod, w, pix, az, feedid, obsids = c4_inputs(n_obs, 0, first=21 + rank * n_obs)
            dd = D.DeviceDestriper(pix, tod, w, 50, 480 * 480, 0, map_shape=(480, 480), ground=(az, feedid, obsids))
            g = dd.gops
            drivers = {'ground_batched': lambda: D.cg_solve_batched(g, D.torch_allreduce, 0.0, niter)[1][0],
                       'ground_eager': lambda: D.cg_solve(g, D.torch_allreduce, 0.0, niter)[1]}
            for fn in drivers.values():
                fn()
            ms = {k: [] for k in drivers}
            for _ in range(rounds):
                for k, fn in drivers.items():
                    dist.barrier()
                    it, dt = timed(fn)
                    assert it == niter, (k, it)
                    ms[k].append(dt / niter * 1e3)
            every = [None] * world
            dist.all_gather_object(every, ms)
            med = {k: statistics.median(v) for k, v in every[0].items()}
            out.append({'mode': 'ranks', 'backend': backend, 'ranks': world, 'gpus': 1,
                        'observations_per_rank': n_obs, 'n_offsets_rank0': dd.ops.n_offsets, 'groups_rank0': g.K,
                        'map_pixels_reduced': dd.ops.npix, 'niter': niter, 'ms_per_iter': med,
                        'ms_per_iter_all_ranks': every,
                        'batched_over_eager': med['ground_batched'] / med['ground_eager']})
            del dd, g, drivers
        dist.barrier()
        dist.destroy_process_group()
        if rank == 0:
            q.put(('ok', out))
    except Exception as e:  # noqa: BLE001
        q.put(('failed', f'{type(e).__name__}: {e}'))


def measure_ranks(world, backend, obs, niter, rounds, limit=600):
    """The ranks mode on one backend: JSON-able records, or one record saying why it did not run."""
    import queue
    import socket
    import torch.multiprocessing as mp
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    procs = [ctx.Process(target=_ranks_worker, args=(r, world, port, backend, obs, niter, rounds, q))
             for r in range(world)]
    for p in procs:
        p.start()
    try:
        status, value = q.get(timeout=limit)
    except queue.Empty:
        status, value = 'failed', f'no answer within {limit} s'
    for p in procs:
        p.join(timeout=30 if status == 'ok' else 5)
        if p.is_alive():
            p.terminate()
            p.join(timeout=30)
    if status == 'ok':
        return value
    return [{'mode': 'ranks', 'backend': backend, 'ranks': world, 'gpus': 1, 'not_run': value}]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--obs', type=int, nargs='+', default=[1, 8])
    ap.add_argument('--niter', type=int, default=100)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--calls', type=int, default=200)
    ap.add_argument('--out', default=None)
    ap.add_argument('--ranks', type=int, default=0, help='ranks mode: this many processes on one GPU')
    ap.add_argument('--backends', nargs='+', default=['gloo', 'nccl'])
    ap.add_argument('--limit', type=int, default=600, help='ranks mode: seconds before a backend counts as not running')
    a = ap.parse_args()
    if a.ranks > 1:
        lines = [json.dumps(r) for b in a.backends for r in measure_ranks(a.ranks, b, a.obs, a.niter, a.rounds, a.limit)]
    else:
        import torch
        device = torch.cuda.current_device()
        lines = [json.dumps(measure(n, a.niter, a.rounds, a.calls, device)) for n in a.obs]
    for line in lines:
        print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
