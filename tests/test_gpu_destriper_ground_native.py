"""The native ground solve (comap_destripe_ground_solve, the default of DeviceDestriper.solve with
``ground=...``) against the eager ``cg_solve`` driver on the same problem
(COMAP_DS_GROUND_SOLVE=eager, read at solve time), and the azimuth wrap of the ground set-up
against the NumPy ``Reference`` of test_gpu_destriper_ground.py on a pre-unwrapped copy.

Cases A and B are that file's; case C has K = 300 groups, so the 2K = 600 tail values pass one
256-thread sweep of the tail code, on 9000 samples.  Tolerance: the project's RTOL = 1e-5 on
relmax (which also requires equal NaN patterns); bit-identity where the issue states it."""
import contextlib
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_destriper_ground as G  # noqa: E402

pytestmark = pytest.mark.gpu

RTOL = G.RTOL
CASES = {'a': G.CASE_A, 'b': G.CASE_B,
         'c': dict(L=10, n_obs=20, n_feeds=15, absent=None, n_off=3, ny=16, nx=16, seed=7)}


@contextlib.contextmanager
def env(**kw):
    old = {k: os.environ.get(k) for k in kw}
    try:
        for k, v in kw.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def problem(case, az=None, **kw):
    from comapreduce_amd.mapmaking.destriper import DeviceDestriper
    return DeviceDestriper(case['pix'], case['tod'], case['w'], case['L'], case['npix'],
                           ground=(case['az'] if az is None else az, case['feed'], case['obs']), **kw)


def solve(dd, mode, threshold, niter, **kw):
    with env(COMAP_DS_GROUND_SOLVE=None if mode == 'native' else mode):
        return dd.solve(threshold, niter, **kw)


def host(v):
    return v if isinstance(v, np.ndarray) else v.cpu().numpy()


_PROBLEMS = {}


@pytest.fixture(scope='module')
def problems():
    """One (case, problem) per case, built on first use and shared: solve() leaves it unchanged."""
    def get(which):
        if which not in _PROBLEMS:
            case = G.make_case(**CASES[which])
            _PROBLEMS[which] = (case, problem(case))
        return _PROBLEMS[which]
    yield get
    _PROBLEMS.clear()


def test_case_c_is_what_it_claims(problems):
    case, dd = problems('c')
    assert dd.gops.K == 300 and case['pix'].size == 9000 and dd.gops.n_offsets == 900 + 600


# ---------------------------------------------------------------- 1. fixed iteration counts
@pytest.mark.parametrize('niter', [1, 5, 16, 17, 40])
@pytest.mark.parametrize('which', ['a', 'b', 'c'])
def test_fixed_iteration_counts_match_eager(which, niter, problems):
    _, dd = problems(which)
    nat, eag = solve(dd, 'native', 0.0, niter), solve(dd, 'eager', 0.0, niter)
    assert nat['iters'] == niter and eag['iters'] == niter
    e_u = G.relmax(host(nat['solution']), host(eag['solution']))
    e_m = G.relmax(host(nat['maps']['map']), host(eag['maps']['map']))
    print(f'case {which} niter {niter}: relmax solution {e_u:.3g}, map {e_m:.3g}')
    assert e_u < RTOL and e_m < RTOL
    for k in ('naive', 'weight', 'hits'):
        assert np.array_equal(host(nat['maps'][k]), host(eag['maps'][k]), equal_nan=True), k


# ---------------------------------------------------------------- 2. stop test
@pytest.mark.parametrize('threshold', [1e-6, 1e-10])
@pytest.mark.parametrize('which', ['a', 'b', 'c'])
def test_stop_iteration_matches_eager(which, threshold, problems):
    _, dd = problems(which)
    nat, eag = solve(dd, 'native', threshold, 1000), solve(dd, 'eager', threshold, 1000)
    print(f"case {which} threshold {threshold:g}: native {nat['iters']}, eager {eag['iters']} iterations")
    assert 1 < nat['iters'] < 1000
    assert nat['iters'] == eag['iters']
    assert G.relmax(host(nat['maps']['map']), host(eag['maps']['map'])) < RTOL


# ---------------------------------------------------------------- 3. stop flags freeze the state
def test_stop_flag_freezes_the_state(problems):
    _, dd = problems('b')
    full = solve(dd, 'native', 1e-6, 1000)
    count = full['iters']
    assert 17 < count < 1000                                  # the stop falls inside a later batch
    exact = solve(dd, 'native', 1e-6, count)
    assert exact['iters'] == count
    assert np.array_equal(host(full['solution']), host(exact['solution']))
    assert np.array_equal(host(full['maps']['map']), host(exact['maps']['map']), equal_nan=True)
    assert solve(dd, 'native', 1e-6, count - 1)['iters'] == count - 1


# ---------------------------------------------------------------- 3b. the batched driver, one rank
@pytest.mark.parametrize('which', ['a', 'b', 'c'])
def test_batched_driver_equals_eager_on_one_rank(which, problems):
    """cg_solve_batched on GroundOps (nb = 1; the driver the ranks use, here without ranks)
    against cg_solve: the same iterates bit for bit.  16 and 17 iterations straddle the
    16-iteration host check."""
    from comapreduce_amd.mapmaking.destriper import cg_solve, cg_solve_batched
    _, dd = problems(which)
    g = dd.gops
    assert (g.K, dd.ops.n_offsets) == {'a': (6, 115), 'b': (4, 1200), 'c': (300, 900)}[which]
    for threshold, niter in ((0.0, 1), (0.0, 16), (0.0, 17), (1e-10, 1000)):
        ub, itb, _, _ = cg_solve_batched(g, lambda t: t, threshold, niter)
        ue, ite, _, _ = cg_solve(g, lambda t: t, threshold, niter)
        print(f'case {which} threshold {threshold:g} niter {niter}: batched {itb}, eager {ite} iterations')
        assert itb == [ite]
        assert ite == niter if threshold == 0.0 else 1 < ite < 1000
        assert np.array_equal(host(ub), host(ue))


# ---------------------------------------------------------------- 4. determinism
def test_native_solve_is_deterministic_with_and_without_the_graph():
    case = G.make_case(**CASES['b'])
    out = {}
    for graph in ('1', '1', '0'):
        with env(COMAP_DS_CGGRAPH=graph):                    # read when the problem is created
            dd = problem(case)
            res = solve(dd, 'native', 1e-9, 40)
        out.setdefault(graph, []).append((host(res['solution']), host(res['maps']['map']), res['iters']))
    first = out['1'][0]
    for u, m, it in (out['1'][1], out['0'][0]):
        assert it == first[2]
        assert np.array_equal(u, first[0]) and np.array_equal(m, first[1], equal_nan=True)


# ---------------------------------------------------------------- 5. zero right-hand side
def test_zero_right_hand_side():
    case = dict(G.make_case(**CASES['a']))
    case['tod'] = np.zeros_like(case['tod'])
    dd = problem(case)
    nat, eag = solve(dd, 'native', 1e-6, 100), solve(dd, 'eager', 1e-6, 100)
    assert nat['iters'] == 1 and eag['iters'] == 1
    assert np.array_equal(np.isnan(host(nat['solution'])), np.isnan(host(eag['solution'])))


# ---------------------------------------------------------------- 6. tiled layout, host delivery
def test_tiled_layout_and_host_delivery(problems):
    from comapreduce_amd.mapmaking.destriper import DeviceDestriper
    case, dd = problems('a')
    # Converged solves (the settings of test_converged_solve_matches_pinv, 1.4e-10 from the pinv
    # map there): the two layouts sum in different orders, CG on this singular operator magnifies
    # such rounding by many orders within its first iterations (2e-5 between the layouts after 30
    # iterations on the MI355X), and only the converged map is unique.
    want = solve(dd, 'native', 1e-20, 2000)
    plain = DeviceDestriper(case['pix'], case['tod'], case['w'], case['L'], case['npix'],
                            map_shape=(12, 12)).solve(1e-20, 2000)
    tiled = problem(case, map_shape=(12, 12))
    for to_host in (False, True):
        res = solve(tiled, 'native', 1e-20, 2000, to_host=to_host)
        assert isinstance(res['maps']['map'], np.ndarray) == to_host
        assert 1 < res['iters'] < 2000 and res['maps']['map'].shape == (case['npix'],)
        for k in ('map', 'naive', 'weight', 'hits'):
            assert G.relmax(host(res['maps'][k]), host(want['maps'][k])) < RTOL, k
        for k in ('hits', 'weight', 'naive', 'map2'):
            assert np.array_equal(host(res['maps'][k]), host(plain['maps'][k]), equal_nan=True), k


# ---------------------------------------------------------------- 7. ABI
def test_abi_rejects_bad_arguments(problems):
    from comapreduce_amd import _native as N
    assert {'comap_destripe_ground_solve', 'comap_destripe_ground_wrapped'} <= set(N.EXPORTED)
    _, dd = problems('a')
    g = dd.gops
    u = g.zeros(g.n_offsets)
    it = ctypes.c_int32(-7)
    lib = N.lib()
    N.bind_stream(g.ctx, g.dev)
    assert lib.comap_destripe_ground_solve(g.g, 1e-6, -1, N.dptr(u), None, None, None, None, ctypes.byref(it)) == -1
    assert lib.comap_destripe_ground_solve(g.g, 1e-6, 10, None, None, None, None, None, ctypes.byref(it)) == -1
    assert lib.comap_destripe_ground_solve(None, 1e-6, 10, N.dptr(u), None, None, None, None, ctypes.byref(it)) == -1
    assert lib.comap_destripe_ground_wrapped(g.g, None) == -1
    assert it.value == -7 and not np.any(host(u))
    # every map pointer may be NULL
    assert lib.comap_destripe_ground_solve(g.g, 0.0, 3, N.dptr(u), None, None, None, None, ctypes.byref(it)) == 0
    assert it.value == 3 and np.any(host(u))


# ---------------------------------------------------------------- 8. azimuth wrap at 0 / 360
def test_groups_across_north_are_unwrapped(problems):
    from comapreduce_amd.mapmaking.destriper import ground_groups
    case, _ = problems('a')
    gid, _, _ = ground_groups(case['feed'], case['obs'], case['L'])
    grp = np.repeat(gid.astype(np.int64), case['L'])
    raw = case['az'].copy()
    raw[grp == 0] = (raw[grp == 0] + 179.0) % 360.0
    raw[grp == 3] = (raw[grp == 3] - 190.5) % 360.0
    moved = (grp == 0) | (grp == 3)
    for k in (0, 3):
        v = raw[grp == k]
        assert v.max() - v.min() > 359.0 and 0.4 < np.mean(v < 180.0) < 0.6
    unwrapped = np.where(moved & (raw < 180.0), raw + 360.0, raw)
    ref = G.Reference(dict(case, az=unwrapped), gid)
    a, b = problem(case, az=raw), problem(case, az=unwrapped)
    np.testing.assert_allclose(host(a.gops.mu), ref.mu, rtol=1e-13)
    np.testing.assert_allclose(host(a.gops.sigma), ref.sigma, rtol=1e-11)
    assert np.all(ref.sigma[[0, 3]] < 10.0) and np.all(ref.mu[[0, 3]] > 180.0)
    ra, rb = solve(a, 'native', 1e-12, 1000), solve(b, 'native', 1e-12, 1000)
    want = np.zeros(6, bool)
    want[[0, 3]] = True
    assert np.array_equal(ra['ground']['wrapped'].reshape(-1), want) and ra['ground']['wrapped'].dtype == bool
    assert ra['ground']['wrapped'].shape == (2, 3) and not np.any(rb['ground']['wrapped'])
    assert ra['iters'] == rb['iters'] and 1 < ra['iters'] < 1000
    assert np.array_equal(host(ra['solution']), host(rb['solution']))
    assert np.array_equal(host(ra['maps']['map']), host(rb['maps']['map']), equal_nan=True)
    for k in ('slope', 'level'):
        assert np.array_equal(ra['ground'][k], rb['ground'][k]), k
    # the eager driver sees the same set-up
    ea = solve(a, 'eager', 1e-12, 1000)
    assert G.relmax(host(ea['maps']['map']), host(ra['maps']['map'])) < RTOL


# ---------------------------------------------------------------- 9. unwrapped groups unchanged
def test_groups_inside_one_turn_keep_their_statistics(problems):
    from comapreduce_amd import _native as N
    case, dd = problems('a')
    res = solve(dd, 'native', 1e-6, 100)
    assert not np.any(res['ground']['wrapped']) and not np.any(host(dd.gops.wrapped))
    with env(COMAP_DS_GROUND_SOLVE='eager'):
        other = problem(case)
        g = other.gops
        mu, sigma = g.zeros(g.K), g.zeros(g.K)
        N.bind_stream(g.ctx, g.dev)
        assert N.lib().comap_destripe_ground_stats(g.g, N.dptr(mu), N.dptr(sigma)) == 0
    assert np.array_equal(host(dd.gops.mu), host(mu)) and np.array_equal(host(dd.gops.sigma), host(sigma))
    from comapreduce_amd.mapmaking.destriper import ground_groups
    gid, _, _ = ground_groups(case['feed'], case['obs'], case['L'])
    ref = G.Reference(case, gid)
    np.testing.assert_allclose(host(dd.gops.mu), ref.mu, rtol=1e-13)
    np.testing.assert_allclose(host(dd.gops.sigma), ref.sigma, rtol=1e-11)
