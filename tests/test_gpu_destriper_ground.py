"""Ground (azimuth) template in the destriper's CG: the device operator (GroundOps,
comap_destripe_ground_*) against a NumPy reference built here from the definition
A = [F G]^T W Z [F G] at the sample level (the reference's op_Ax_with_ground,
Destriper.py:265-336, with the azimuth centred and scaled per group).

Case A (every branch at the smallest size): L = 10, 2 observations x 3 feeds with one
combination absent, 23 offsets per group, a 12 x 12 map, ~3% of the samples at pixel -1
or -5, 5% zero weights, one group with a constant azimuth (sigma = 0), per-sample weights
(the f64 entry form), and the last map row reached only through the negative ids' wrap.
Case B (multi-chunk group rows): L = 50, K = 4, 60 000 samples, a 64 x 64 map, one weight
per group (the count entry form); every group row holds thousands of (group, pixel)
entries, i.e. several reduction chunks.

Bounds.  Test 1 uses |dev - ref|_i <= 8 N 2^-53 B_i with B the same pipeline on absolute
values, B = |Fm|^T (w (|Fm||p| + P H^-1 P^T (w |Fm||p|))): the worst-case reordering error
of sums of at most N terms.  Test 2 uses the project's RTOL = 1e-5 with relmax; the
largest relmax seen on the MI355X is recorded in DESIGN.md."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RTOL = 1e-5
EPS = 2.0 ** -53


def relmax(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    fin = np.isfinite(b)
    assert np.array_equal(np.isfinite(a), fin), 'NaN pattern differs'
    return np.max(np.abs(a[fin] - b[fin])) / max(np.max(np.abs(b[fin])), 1e-300)


# ---------------------------------------------------------------- inputs
def make_case(L, n_obs, n_feeds, absent, n_off, ny, nx, seed, const_group=None, group_weights=False,
              inject=False, xf=3.3):
    """Samples of n_obs x n_feeds groups (minus `absent`), n_off offsets each, scanning the
    rows 0 .. ny - 2 of an ny x nx map (the last row is only ever read through the wrap)."""
    rng = np.random.default_rng(seed)
    npix = ny * nx
    obs_ids, feed_ids = 100 + 7 * np.arange(n_obs), 1 + 3 * np.arange(n_feeds)
    pix, az, obs, feed, wgt = [], [], [], [], []
    n = n_off * L
    t = np.arange(n)
    for i in range(n_obs):
        for j in range(n_feeds):
            if (i, j) == absent:
                continue
            k = i * n_feeds + j
            x = (nx - 1) * (0.5 + 0.5 * np.sin(2 * np.pi * t / (n / (xf + k)) + 0.7 * k))
            y = (ny - 2) * (0.5 + 0.5 * np.sin(2 * np.pi * t / (n / (1.7 + 0.37 * k)) + 1.3 * k))
            pix.append(np.rint(y).astype(np.int64) * nx + np.rint(x).astype(np.int64))
            a = 180.0 + 4.0 * k + 6.0 * np.sin(2 * np.pi * t / (n / (5.1 + 0.61 * k)) + 0.4 * k) \
                + 0.3 * rng.standard_normal(n)
            az.append(np.full(n, 151.25 + k) if k == const_group else a)
            obs.append(np.full(n, obs_ids[i]))
            feed.append(np.full(n, feed_ids[j]))
            wgt.append(np.full(n, 0.5 + rng.random()) if group_weights else 0.5 + rng.random(n))
    pix, az, obs, feed, w = (np.concatenate(v) for v in (pix, az, obs, feed, wgt))
    N = pix.size
    off = rng.random(N) < 0.03                       # unbinned samples: they read m[npix + p]
    pix[off] = np.where(rng.random(int(off.sum())) < 0.5, -1, -5)
    w[rng.random(N) < 0.05] = 0.0
    tod = rng.standard_normal(N)
    truth = None
    if inject:
        sky = 2.0 * rng.standard_normal(npix)
        grp = (np.searchsorted(obs_ids, obs) * n_feeds + np.searchsorted(feed_ids, feed))
        drift = np.repeat(np.cumsum(0.3 * rng.standard_normal(N // L)), L)
        slope, level = 0.6 * rng.standard_normal(n_obs * n_feeds), rng.standard_normal(n_obs * n_feeds)
        tod = sky[pix % npix] + drift + slope[grp] * (az - 180.0) + level[grp] + 0.1 * rng.standard_normal(N)
        truth = sky
    return {'L': L, 'npix': npix, 'pix': pix.astype(np.int32), 'az': az, 'obs': obs, 'feed': feed, 'w': w,
            'tod': tod, 'K': n_obs * n_feeds, 'sky': truth}


# ---------------------------------------------------------------- the NumPy reference
class Reference:
    """A = [F G]^T W Z [F G] from its definition, sample by sample.  Vectors are
    [x (N/L, the caller's offset order) | s (K) | c (K)]."""

    def __init__(self, case, gid):
        self.L, self.npix, self.K = case['L'], case['npix'], case['K']
        self.pix, self.w, self.tod = case['pix'].astype(np.int64), case['w'], case['tod']
        az = case['az']
        self.N = self.pix.size
        self.NO = self.N // self.L
        self.off = np.arange(self.N) // self.L
        self.grp = np.asarray(gid, np.int64)[self.off]
        self.mu, self.sigma = np.zeros(self.K), np.zeros(self.K)
        for k in range(self.K):
            v = az[self.grp == k]
            if v.size:
                self.mu[k] = v.mean()
                self.sigma[k] = 0.0 if v.max() == v.min() else np.sqrt(np.mean((v - self.mu[k]) ** 2))
        sg = self.sigma[self.grp]
        self.a = np.where(sg > 0, (az - self.mu[self.grp]) / np.where(sg > 0, sg, 1.0), 0.0)
        self.binned = self.pix >= 0
        self.read = np.where(self.binned, self.pix, self.npix + self.pix)     # m[pointing]'s wrap
        self.h = self.bin(self.w)
        self.hits = np.bincount(self.pix[self.binned], minlength=self.npix).astype(float)

    def bin(self, v):
        return np.bincount(self.pix[self.binned], weights=v[self.binned], minlength=self.npix)

    def share(self, num):
        return np.where(self.h != 0, num / np.where(self.h != 0, self.h, 1.0), num)

    def split(self, u):
        return u[:self.NO], u[self.NO:self.NO + self.K], u[self.NO + self.K:]

    def template(self, u, absolute=False):
        x, s, c = self.split(np.abs(u) if absolute else u)
        return x[self.off] + s[self.grp] * (np.abs(self.a) if absolute else self.a) + c[self.grp]

    def adjoint(self, v, absolute=False):
        a = np.abs(self.a) if absolute else self.a
        return np.concatenate([np.bincount(self.off, weights=v, minlength=self.NO),
                               np.bincount(self.grp, weights=v * a, minlength=self.K),
                               np.bincount(self.grp, weights=v, minlength=self.K)])

    def Z(self, z):
        return z - self.share(self.bin(self.w * z))[self.read]

    def A(self, u):
        return self.adjoint(self.w * self.Z(self.template(u)))

    def b(self):
        return self.adjoint(self.w * self.Z(self.tod))

    def bound(self, u=None):
        """B of the module docstring for A u (u = None: for b, |Fm||p| -> |tod|)."""
        t = np.abs(self.tod) if u is None else self.template(u, absolute=True)
        return self.adjoint(self.w * (t + self.share(self.bin(self.w * t))[self.read]), absolute=True)

    def dense(self):
        n = self.NO + 2 * self.K
        return np.stack([self.A(e) for e in np.eye(n)], axis=1)

    def destriped(self, u):
        return self.share(self.bin(self.w * (self.tod - self.template(u))))


def device_ops(case):
    from comapreduce_amd.mapmaking.destriper import DeviceOps, GroundOps, ground_groups
    gid, uobs, ufeed = ground_groups(case['feed'], case['obs'], case['L'])
    ops = DeviceOps(case['pix'], case['tod'], case['w'], case['L'], case['npix'])
    return GroundOps(ops, case['az'], gid, uobs.size * ufeed.size), gid


def internal_position(g):
    """pos[o] = internal position of the caller's offset o."""
    import torch
    k = torch.arange(g.NO, dtype=torch.float64, device=g.dev)
    return g.ops.natural(k).cpu().numpy().astype(np.int64)


def to_internal(g, pos, u):
    import torch
    v = np.array(u, dtype=np.float64)
    v[:g.NO][pos] = u[:g.NO]
    return torch.from_numpy(v).to(g.dev)


def to_natural(g, pos, t):
    v = t.cpu().numpy()
    out = v.copy()
    out[:g.NO] = v[:g.NO][pos]
    return out


CASE_A = dict(L=10, n_obs=2, n_feeds=3, absent=(1, 1), n_off=23, ny=12, nx=12, seed=11, const_group=2)
CASE_B = dict(L=50, n_obs=2, n_feeds=2, absent=None, n_off=300, ny=64, nx=64, seed=5, group_weights=True, xf=31.3)


@pytest.fixture(scope='module')
def case_a():
    case = make_case(**CASE_A)
    g, gid = device_ops(case)
    return case, Reference(case, gid), g


@pytest.fixture(scope='module')
def case_b():
    case = make_case(**CASE_B)
    g, gid = device_ops(case)
    return case, Reference(case, gid), g


def test_cases_exercise_what_they_claim(case_a, case_b):
    case, ref, g = case_a
    assert ref.K == 6 and ref.NO == 5 * 23 and not np.any(ref.grp == 4)          # one combination absent
    assert ref.sigma[2] == 0.0 and np.all(ref.sigma[[0, 1, 3, 5]] > 0)
    assert 0.01 < np.mean(~ref.binned) < 0.06 and {-1, -5} <= set(case['pix'][~ref.binned].tolist())
    assert 0.02 < np.mean(case['w'] == 0) < 0.09
    last = np.arange(ref.npix - 12, ref.npix)
    assert np.all(ref.hits[last] == 0) and np.any(ref.read == ref.npix - 1)       # hit only through the wrap
    np.testing.assert_allclose(g.mu.cpu().numpy(), ref.mu, rtol=1e-13)
    np.testing.assert_allclose(g.sigma.cpu().numpy(), ref.sigma, rtol=1e-11)
    assert float(g.sigma[2]) == 0.0
    case, ref, g = case_b
    assert ref.N == 60_000 and ref.K == 4
    nnz, nnzb = g.nnz()
    assert nnz / 4 > 2 * 1024 and 0 < nnzb < nnz          # every group row spans several 1024-entry chunks
    assert g.ops.entry_bytes() == 5                        # the count entry form; case A: f64 weights
    assert case_a[2].ops.entry_bytes() == 12


@pytest.mark.parametrize('which', ['a', 'b'])
def test_matvec_and_rhs_within_reordering_bound(which, case_a, case_b):
    case, ref, g = case_a if which == 'a' else case_b
    pos = internal_position(g)
    rng = np.random.default_rng(3)
    p = rng.standard_normal(g.n_offsets)
    h, _, nnum = g.local_maps()
    num, q, b = g.zeros(g.npix), g.zeros(g.n_offsets), g.zeros(g.n_offsets)
    pd = to_internal(g, pos, p)
    g.bin(pd, 0, num)
    g.project(pd, num, h, q)
    g.project(None, nnum, h, b)
    tol = 8 * ref.N * EPS
    for name, dev, want, bnd in (('A p', q, ref.A(p), ref.bound(p)), ('b', b, ref.b(), ref.bound())):
        err = np.abs(to_natural(g, pos, dev) - want)
        ratio = float(np.max(err / np.maximum(tol * bnd, 1e-300)))
        print(f'case {which} {name}: max |dev - ref| / (8 N eps B) = {ratio:.3g}')
        assert np.all(err <= tol * bnd), (name, ratio)
    # the fused p.q of project() is the dot product of the whole vector
    dot = g.scalar()
    g.project(pd, num, h, q, dot)
    assert abs(float(dot) - float(p @ ref.A(p))) <= 1e-10 * float(np.abs(p) @ ref.bound(p))


def test_converged_solve_matches_pinv(case_a):
    from comapreduce_amd.mapmaking.destriper import DeviceDestriper
    case, ref, _ = case_a
    u_ref = np.linalg.pinv(ref.dense(), rcond=1e-12, hermitian=True) @ ref.b()
    dd = DeviceDestriper(case['pix'], case['tod'], case['w'], case['L'], case['npix'],
                         ground=(case['az'], case['feed'], case['obs']))
    res = dd.solve(threshold=1e-20, niter=2000)
    pos = internal_position(dd.gops)
    u = to_natural(dd.gops, pos, res['solution'])
    hit = ref.hits > 0
    e_map = relmax(res['maps']['map'].cpu().numpy()[hit], ref.destriped(u_ref)[hit])
    e_res = relmax(ref.Z(ref.template(u)), ref.Z(ref.template(u_ref)))
    print(f"iterations {res['iters']}, relmax map {e_map:.3g}, relmax Z[F G]x {e_res:.3g}")
    assert res['iters'] < 2000
    assert e_map < RTOL and e_res < RTOL
    assert np.array_equal(res['x'].cpu().numpy(), u[:ref.NO])
    # the fit in the reference's units: slope = s / sigma, level = c - s mu / sigma
    s, c = u[ref.NO:ref.NO + ref.K], u[ref.NO + ref.K:]
    ok = ref.sigma > 0
    slope = np.where(ok, s / np.where(ok, ref.sigma, 1.0), 0.0)
    gr = res['ground']
    assert gr['slope'].shape == gr['level'].shape == (2, 3)
    np.testing.assert_allclose(gr['slope'].reshape(-1), slope, rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(gr['level'].reshape(-1), c - slope * ref.mu, rtol=1e-9, atol=1e-9)
    assert gr['slope'][0, 2] == 0.0                  # the constant-azimuth group
    assert gr['slope'][1, 1] == 0.0 and gr['level'][1, 1] == 0.0     # the absent combination


def test_ground_fit_improves_the_map():
    from comapreduce_amd.mapmaking.destriper import DeviceDestriper
    case = make_case(L=10, n_obs=2, n_feeds=3, absent=(1, 1), n_off=60, ny=12, nx=12, seed=21, inject=True)
    args = (case['pix'], case['tod'], case['w'], case['L'], case['npix'])
    plain = DeviceDestriper(*args).solve(threshold=1e-12, niter=1000)
    ground = DeviceDestriper(*args, ground=(case['az'], case['feed'], case['obs'])).solve(threshold=1e-12, niter=1000)
    hit = plain['maps']['hits'].cpu().numpy() > 0

    def rms(res):
        d = (res['maps']['map'].cpu().numpy() - case['sky'])[hit]
        return float(np.std(d - d.mean()))
    print(f'map rms error: ground {rms(ground):.3g}, plain {rms(plain):.3g}')
    assert rms(ground) < rms(plain)


def test_ground_solve_is_deterministic(case_b):
    from comapreduce_amd.mapmaking.destriper import DeviceDestriper
    case = case_b[0]
    out = []
    for _ in range(2):
        dd = DeviceDestriper(case['pix'], case['tod'], case['w'], case['L'], case['npix'],
                             ground=(case['az'], case['feed'], case['obs']))
        res = dd.solve(threshold=1e-9, niter=40)
        out.append((res['solution'].cpu().numpy(), res['maps']['map'].cpu().numpy(), res['iters']))
    assert out[0][2] == out[1][2]
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])


def test_off_means_off_and_interfaces(case_a):
    from comapreduce_amd.mapmaking.destriper import DeviceDestriper, run_destriper
    case = case_a[0]
    args = (case['pix'], case['tod'], case['w'], case['L'], case['npix'])
    r0 = DeviceDestriper(*args).solve(1e-6, 100)
    r1 = DeviceDestriper(*args, ground=None).solve(1e-6, 100)
    assert 'ground' not in r0 and 'ground' not in r1 and r0['iters'] == r1['iters']
    assert np.array_equal(r0['x'].cpu().numpy(), r1['x'].cpu().numpy())
    for k in r0['maps']:
        assert np.array_equal(r0['maps'][k].cpu().numpy(), r1['maps'][k].cpu().numpy(), equal_nan=True), k
    out = run_destriper(case['pix'], case['tod'], case['w'], case['L'], np.arange(case['npix']), az=case['az'],
                        feedid=case['feed'], obsids=case['obs'], ground=True)
    assert set(out) == {'All', 'Ground'}
    assert out['Ground']['slope'].shape == out['Ground']['level'].shape == (2, 3)
    assert np.array_equal(out['Ground']['obsids'], np.unique(case['obs']))
    assert np.array_equal(out['Ground']['feeds'], np.unique(case['feed']))
    assert {'map', 'naive', 'weight', 'map2', 'hits'} <= set(out['All']) and out['All']['map'].shape == (case['npix'],)
    two = np.stack([case['tod'], case['tod']])
    with pytest.raises(NotImplementedError):
        DeviceDestriper(case['pix'], two, np.stack([case['w'], case['w']]), case['L'], case['npix'],
                        ground=(case['az'], case['feed'], case['obs']))


def test_main_writes_the_ground_fit(tmp_path):
    """run_destriper.main(ground=True): the per-band loop on the tiled map layout, the FITS
    maps as without the fit, and the fit in <prefix>_ground_band<iband>.npz."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
    import comapdata_case as cc
    from comapreduce_amd.mapmaking.run_destriper import main
    store, names = cc.store()
    m = cc.CASES['car']['map']
    kw = dict(offset_length=50, prefix='t', feeds=cc.FEEDS, nxpix=m['nxpix'], nypix=m['nypix'], crval=m['crval'],
              crpix=m['crpix'], ctype=m['ctype'], cdelt=m['cdelt'], use_gain_filter=True, calibration=False,
              threshold=1e-6, niter=50, bands=(0,), store=store)
    plain = main(names[:2], output_dir=str(tmp_path / 'plain'), **kw)[0]
    out = main(names[:2], output_dir=str(tmp_path / 'ground'), ground=True, **kw)[0]
    assert set(out) == {'All', 'Ground'} and set(plain) == {'All'}
    for k in ('weight', 'hits', 'naive'):
        assert np.array_equal(out['All'][k], plain['All'][k], equal_nan=True), k
    assert np.all(np.isfinite(out['All']['map'][out['All']['hits'] > 0]))
    assert os.path.exists(tmp_path / 'ground' / 'All_t_Band00.fits')
    fit = np.load(tmp_path / 'ground' / 't_ground_band0.npz')
    gr = out['Ground']
    assert gr['slope'].shape == (gr['obsids'].size, gr['feeds'].size) and np.all(np.isfinite(gr['slope']))
    for k in ('obsids', 'feeds', 'slope', 'level'):
        assert np.array_equal(fit[k], gr[k]), k
    assert not os.path.exists(tmp_path / 'plain' / 't_ground_band0.npz')
