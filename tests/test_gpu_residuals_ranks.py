"""Residual chi-squared across ranks: DeviceDestriper(residual_cut=...) and run_destriper(residuals=
True) sharded over 2 gloo ranks that share cuda:0.  Each rank passes its own samples and offsets
against the global map; the group sums and counts are added across ranks over the union of the
ranks' (observation, feed) groups, so every rank holds the same table and takes the same cut.

The noisy case of test_gpu_residuals.py on case B's geometry, split by observation: each rank holds
whole (observation, feed) groups, so a group has one contributing rank and the all-reduced sum is
that rank's own sum bit for bit.  Every test spawns its two ranks once; the time limit covers both
ranks, start-up included."""
import os
import queue
import socket
import sys
import traceback

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_destriper_ground as G  # noqa: E402
import test_gpu_residuals as T  # noqa: E402

pytestmark = pytest.mark.gpu

TIME_LIMIT = 240
CUT = 5.0


# ---------------------------------------------------------------- the two ranks
def _job_tables(rank, parts, npix):
    """The rank's DeviceDestriper(residual_cut=CUT) solve -- tables, offsets and the (shared) map as
    host arrays -- and run_destriper(residuals=True)'s 'Residuals'."""
    from comapreduce_amd.mapmaking.destriper import DeviceDestriper, run_destriper
    c = parts[rank]
    dd = DeviceDestriper(c['pix'], c['tod'], c['w'], c['L'], npix, device=0, map_shape=(64, 64),
                         residual_groups=(c['feed'], c['obs']), residual_cut=CUT)
    res = dd.solve(1e-6, 100)
    out = {k: v.cpu().numpy() for k, v in res['residuals'].items()}
    out.update(x=res['x'].cpu().numpy(), map=res['maps']['map'].cpu().numpy(), hits=res['maps']['hits'].cpu().numpy(),
               axes=dd.resid_axes)
    drv = run_destriper(c['pix'], c['tod'], c['w'], c['L'], np.arange(npix), feedid=c['feed'], obsids=c['obs'],
                        device=0, map_shape=(64, 64), residuals=True, threshold=1e-6, niter=100)
    out['driver'] = (sorted(drv), drv['Residuals'], drv['All']['map'] is None)
    return out


def _job_errors(rank, parts, npix):
    """DEVICE labels, rank 1's out of range: only the pass itself sees that, at solve time."""
    import torch
    from comapreduce_amd.mapmaking.destriper import DeviceDestriper
    c = parts[rank]
    lab = torch.zeros(c['pix'].size // c['L'], dtype=torch.int32, device='cuda:0')
    if rank == 1:
        lab[3] = 2
    try:
        DeviceDestriper(c['pix'], c['tod'], c['w'], c['L'], npix, device=0, residuals=(lab, 2)).solve(1e-6, 10)
        return None
    except Exception as e:  # noqa: BLE001
        return type(e).__name__, str(e)


_JOBS = {'tables': _job_tables, 'errors': _job_errors}


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
    """Both ranks' results of one job; a rank that fails or does not answer inside the time limit
    fails the test (the children are terminated, nothing is retried)."""
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


# ---------------------------------------------------------------- inputs
def parts_by_observation():
    """(case, tod, w, gid, G, [each rank's part, 'gid' = its offsets' global groups, 'at' = its samples])."""
    case, tod, w, gid, n_groups = T.noisy_case(G.CASE_B)
    uobs = np.unique(case['obs'])
    assert uobs.size == 2 and n_groups == 4
    L = case['L']
    parts = []
    for o in uobs:
        i = np.nonzero(case['obs'] == o)[0]
        assert np.array_equal(i, np.arange(i[0], i[-1] + 1)) and i[0] % L == 0 and np.unique(case['feed'][i]).size == 2
        parts.append(dict(pix=case['pix'][i], tod=tod[i], w=w[i], feed=case['feed'][i], obs=case['obs'][i], L=L,
                          gid=gid[i[0] // L:(i[-1] + 1) // L], at=i))
    assert sorted(set(parts[0]['gid'])) == [0, 1] and sorted(set(parts[1]['gid'])) == [2, 3]
    return case, tod, w, gid, n_groups, parts


# ---------------------------------------------------------------- 1. the tables and the cut
def test_two_ranks_share_one_table_and_one_cut():
    from comapreduce_amd.mapmaking.destriper import DeviceDestriper
    case, tod, w, gid, n_groups, parts = parts_by_observation()
    npix, L = case['npix'], case['L']
    send = [{k: v for k, v in p.items() if k not in ('gid', 'at')} for p in parts]
    r0, r1 = run_ranks('tables', send, npix)
    # one table, one decision, one map
    want_cut = np.arange(n_groups) == n_groups - 1
    for k in ('chi2', 'sum', 'count', 'cut', 'chi2_first'):
        assert np.array_equal(r0[k], r1[k]), k
    assert np.array_equal(r0['cut'], want_cut) and r0['cut'].dtype == bool
    assert np.array_equal(r0['map'], r1['map'], equal_nan=True) and np.array_equal(r0['hits'], r1['hits'])
    for r in (r0, r1):
        assert r['axes'][0].tolist() == np.unique(case['obs']).tolist()          # the union of the ranks' observations
        assert r['axes'][1].tolist() == np.unique(case['feed']).tolist()
    # each rank's own pass, restated from its own x and the shared map (after the cut: the last group
    # has zero weights and dropped offsets); whole groups per rank: the all-reduced sum is the owner's
    for part, r in zip(parts, (r0, r1)):
        gone = part['gid'] == n_groups - 1
        w_cut = np.where(np.repeat(gone, L), 0.0, part['w'])
        want = T.restate(part['pix'], part['tod'], w_cut, r['x'], r['map'], L, part['gid'], n_groups,
                         keep=(~gone).astype(np.uint8))
        assert np.array_equal(r['offset_sum'], want[0]) and np.array_equal(r['offset_count'], want[1])
        mine = np.unique(part['gid'])
        assert np.array_equal(r0['sum'][mine], want[2][mine]) and np.array_equal(r0['count'][mine], want[3][mine])
        assert np.all(want[3][np.setdiff1d(np.arange(n_groups), mine)] == 0)
    assert r0['count'][n_groups - 1] == 0 and np.all(r0['count'][:n_groups - 1] > 0)
    # the single-rank run: the same counts and decision; the offsets of a sharded and a single-rank
    # CG differ in the last bits, so chi2 is held to the project's bound for two solves of one system
    one = DeviceDestriper(case['pix'], tod, w, L, npix, map_shape=(64, 64), residual_groups=(case['feed'], case['obs']),
                          residual_cut=CUT).solve(1e-6, 100)
    s = {k: v.cpu().numpy() for k, v in one['residuals'].items()}
    assert np.array_equal(s['count'], r0['count']) and np.array_equal(s['cut'], r0['cut'])
    assert np.array_equal(np.concatenate([r0['offset_count'], r1['offset_count']]), s['offset_count'])
    for k in ('chi2', 'chi2_first'):
        e = G.relmax(r0[k], s[k])
        print(f'{k}: relmax two ranks vs one = {e:.3g}', r0[k], s[k])
        assert e <= G.RTOL
    assert r0['chi2_first'][n_groups - 1] > CUT and np.all(r0['chi2_first'][:n_groups - 1] < CUT)
    # the driver: rank 0 gets the table, the other rank None (and None maps)
    keys0, tab0, none0 = r0['driver']
    keys1, tab1, none1 = r1['driver']
    assert keys0 == keys1 == ['All', 'Residuals'] and tab1 is None and none1 and not none0
    assert set(tab0) == {'obsids', 'feeds', 'chi2', 'count'} and tab0['chi2'].shape == (2, 2)
    assert G.relmax(tab0['chi2'].reshape(-1), s['chi2_first']) <= G.RTOL
    assert int(tab0['count'].sum()) == int(np.sum((case['pix'] >= 0) & (w > 0)))


# ---------------------------------------------------------------- 2. errors arrive on every rank
def test_label_out_of_range_fails_both_ranks():
    case, tod, w, gid, n_groups, parts = parts_by_observation()
    send = [{k: v for k, v in p.items() if k not in ('gid', 'at')} for p in parts]
    res = run_ranks('errors', send, case['npix'])
    for rank in range(2):
        assert res[rank] is not None and res[rank][0] == 'ValueError', (rank, res[rank])
    assert 'label out of range' in res[1][1] and 'rank 1' in res[0][1]
