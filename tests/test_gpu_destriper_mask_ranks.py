"""The solve mask across ranks: DeviceDestriper(solve_mask=...) sharded over 2 gloo ranks that share
cuda:0, on the seed-0 source case of test_gpu_destriper_mask.py split at offset 120.  Each rank builds
the view of its own samples under the one global mask; the sharded CG solves the masked system (h' and
nnum' summed across ranks), the maps are binned from the full problems with their own all-reduce of h
and the naive numerator.  Each rank's offsets equal the single-rank solve's within the project's RTOL
with the same iteration count, and both ranks hold the same maps.  A mask of the wrong length on one
rank raises on both.  Every test spawns its two ranks once."""
import os
import queue
import socket
import sys
import traceback

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_destriper_ground as G  # noqa: E402
import test_gpu_destriper_mask as M  # noqa: E402

pytestmark = pytest.mark.gpu

TIME_LIMIT = 240


def _job_solve(rank, parts, npix, masks):
    from comapreduce_amd.mapmaking.destriper import DeviceDestriper
    c = parts[rank]
    dd = DeviceDestriper(c['pix'], c['tod'], c['w'], c['L'], npix, device=0, map_shape=(12, 12), solve_mask=masks[rank])
    res = dd.solve(1e-14, 300)
    return {'x': res['x'].cpu().numpy(), 'iters': int(res['iters']), 'info': res['solve_mask'],
            'compacted': dd.hit_index is not None, 'maps': {k: v.cpu().numpy() for k, v in res['maps'].items()}}


def _job_errors(rank, parts, npix, masks):
    from comapreduce_amd.mapmaking.destriper import DeviceDestriper
    c = parts[rank]
    try:
        DeviceDestriper(c['pix'], c['tod'], c['w'], c['L'], npix, device=0, map_shape=(12, 12), solve_mask=masks[rank])
        return None
    except Exception as e:  # noqa: BLE001
        return type(e).__name__, str(e)


_JOBS = {'mask_solve': _job_solve, 'mask_errors': _job_errors}


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
    """Both ranks' results of one job (test_gpu_destriper_prior_ranks.run_ranks on this module's jobs): a
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
    c = M.source_case(0)
    n = c['pix'].size // 2
    parts = [dict(pix=c['pix'][s], tod=c['tod'][s], w=c['w'][s], L=c['L']) for s in (slice(0, n), slice(n, None))]
    return c, parts


def test_two_ranks_solve_the_single_rank_masked_system():
    c, parts = halves()
    r0, r1 = run_ranks('mask_solve', parts, c['npix'], [c['mask'], c['mask']])
    one = M.solve_source(c, c['mask'])
    x = np.concatenate([r0['x'], r1['x']])
    e = G.relmax(x, one['x'])
    print(f'two ranks vs one: relmax {e:.3g}; iterations {r0["iters"]}, {r1["iters"]} vs {one["iters"]}')
    assert r0['x'].size == r1['x'].size == 120 and e <= G.RTOL
    assert r0['iters'] == r1['iters'] == one['iters']
    assert np.all(x[c['empty']] == 0.0)
    for k in ('map', 'naive', 'weight', 'hits'):
        assert np.array_equal(r0['maps'][k], r1['maps'][k], equal_nan=True), k
    assert G.relmax(r0['maps']['map'], one['maps']['map']) <= G.RTOL
    for k in ('weight', 'hits'):                                        # the full weights, masked pixels included
        assert np.array_equal(r0['maps'][k], one['maps'][k]), k
    assert np.count_nonzero(r0['maps']['weight'][c['mask']]) == 11      # (two of the 13 are never hit)
    assert r0['info'] == r1['info'] == one['solve_mask']                # counted over both ranks


def test_wrong_length_on_one_rank_fails_both_ranks():
    c, parts = halves()
    res = run_ranks('mask_errors', parts, c['npix'], [c['mask'], c['mask'][:-1]])
    for rank in range(2):
        assert res[rank] is not None and res[rank][0] == 'ValueError', (rank, res[rank])
    assert 'one flag per map pixel' in res[1][1] and 'rank 1' in res[0][1]
