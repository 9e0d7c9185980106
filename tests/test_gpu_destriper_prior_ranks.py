"""The noise prior across ranks: DeviceDestriper(prior=...) sharded over 2 gloo ranks that share
cuda:0.  The solve geometry of test_gpu_destriper_prior.py with its two groups of 120 offsets, one
per rank: T is rank-local, the sharded CG (``cg_solve`` with the all-reduces) solves the same system
as one rank, so each rank's offsets equal the single-rank solve's within the project's RTOL and both
ranks hold the same maps.  A group id with offsets on both ranks, or one rank's group in two runs,
raises on both ranks.  Every test spawns its two ranks once."""
import os
import queue
import socket
import sys
import traceback

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_destriper_ground as G  # noqa: E402
import test_gpu_destriper_prior as P  # noqa: E402

pytestmark = pytest.mark.gpu

TIME_LIMIT = 240


def _job_solve(rank, parts, npix, stencil):
    from comapreduce_amd.mapmaking.destriper import DeviceDestriper
    c = parts[rank]
    dd = DeviceDestriper(c['pix'], c['tod'], c['w'], c['L'], npix, device=0, map_shape=(12, 12),
                         prior=(c['gid'], stencil))
    res = dd.solve(1e-14, 300)
    return {'x': res['x'].cpu().numpy(), 'iters': int(res['iters']),
            'maps': {k: v.cpu().numpy() for k, v in res['maps'].items()}}


def _job_errors(rank, parts, npix, stencil):
    from comapreduce_amd.mapmaking.destriper import DeviceDestriper
    c = parts[rank]
    try:
        DeviceDestriper(c['pix'], c['tod'], c['w'], c['L'], npix, device=0, prior=(c['gid'], stencil))
        return None
    except Exception as e:  # noqa: BLE001
        return type(e).__name__, str(e)


_JOBS = {'prior_solve': _job_solve, 'prior_errors': _job_errors}


def _rank(rank, world, port, q, job, args):
    try:
        import torch
        import torch.distributed as dist
        os.environ['MASTER_ADDR'] = '127.0.0.1'
        os.environ['MASTER_PORT'] = str(port)
        torch.cuda.set_device(0)
        dist.init_process_group('gloo', rank=rank, world_size=world)
        q.put((rank, 'ok', _JOBS[job](rank, *args)))
        dist.barrier()
        dist.destroy_process_group()
    except Exception:  # noqa: BLE001
        q.put((rank, 'failed', traceback.format_exc()))


def run_ranks(job, *args):
    """Both ranks' results of one job (test_gpu_residuals_ranks.run_ranks on this module's jobs): a
    rank that fails or does not answer inside the time limit fails the test; nothing is retried."""
    import torch.multiprocessing as mp
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    procs = [ctx.Process(target=_rank, args=(r, 2, port, q, job, args)) for r in range(2)]
    for p in procs:
        p.start()
    got = {}
    try:
        for _ in range(2):
            rank, status, value = q.get(timeout=TIME_LIMIT)
            assert status == 'ok', f'rank {rank}:\n{value}'
            got[rank] = value
        for p in procs:
            p.join(timeout=60)
        assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
    except queue.Empty:
        pytest.fail(f'ranks {sorted(set(range(2)) - set(got))} did not answer within {TIME_LIMIT} s')
    finally:
        for p in procs:
            if p.is_alive():
                p.terminate()
                p.join(timeout=30)
    return [got[0], got[1]]


def halves():
    c = P.solve_case(0)
    gid, stencil = P.prior_of(2)
    n = c['pix'].size // 2
    parts = [dict(pix=c['pix'][s], tod=c['tod'][s], w=c['w'][s], L=c['L'], gid=gid[g])
             for s, g in ((slice(0, n), slice(0, 120)), (slice(n, None), slice(120, None)))]
    assert set(parts[0]['gid']) == {0} and set(parts[1]['gid']) == {1}
    return c, gid, stencil, parts


def test_two_ranks_solve_the_single_rank_system():
    c, gid, stencil, parts = halves()
    r0, r1 = run_ranks('prior_solve', parts, c['npix'], stencil)
    x1, it1, m1 = P.device_solve(c, (gid, stencil), None)
    x = np.concatenate([r0['x'], r1['x']])
    e = G.relmax(x, x1)
    print(f'two ranks vs one: relmax {e:.3g}; iterations {r0["iters"]}, {r1["iters"]} vs {it1}')
    assert r0['x'].size == r1['x'].size == 120 and e <= G.RTOL
    assert G.relmax(r0['x'], x1[:120]) <= G.RTOL and G.relmax(r1['x'], x1[120:]) <= G.RTOL
    assert r0['iters'] == r1['iters']
    for k in ('map', 'naive', 'weight', 'hits'):
        assert np.array_equal(r0['maps'][k], r1['maps'][k], equal_nan=True), k
    assert G.relmax(r0['maps']['map'], m1['map']) <= G.RTOL
    assert np.array_equal(r0['maps']['hits'], m1['hits'])


def test_group_split_across_ranks_fails_both_ranks():
    c, gid, stencil, parts = halves()
    split = [dict(p) for p in parts]
    split[1]['gid'] = np.where(np.arange(120) < 60, 0, 1).astype(np.int32)
    res = run_ranks('prior_errors', split, c['npix'], stencil)
    for rank in range(2):
        assert res[rank] is not None and res[rank][0] == 'ValueError', (rank, res[rank])
        assert 'ranks 0 and 1' in res[rank][1]


def test_non_contiguous_group_on_one_rank_fails_both_ranks():
    c, gid, stencil, parts = halves()
    runs = [dict(p) for p in parts]
    runs[1]['gid'] = np.where((np.arange(120) >= 40) & (np.arange(120) < 50), -1, 1).astype(np.int32)
    runs[1]['gid'][45] = 1
    res = run_ranks('prior_errors', runs, c['npix'], stencil)
    for rank in range(2):
        assert res[rank] is not None and res[rank][0] == 'ValueError', (rank, res[rank])
    assert 'more than one run' in res[1][1] and 'rank 1' in res[0][1]
