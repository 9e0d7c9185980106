"""Solve mask for the destriper (comap_destripe_mask_view / _solve_view, DeviceOps.masked_view,
DeviceDestriper(solve_mask=...), the driver's solve_mask): the offsets are fitted from the samples
outside a pixel mask, w' = 0 where the pixel is masked, and every output after the CG uses the full w.

1. the view against the definition: h' / nnum' are the parent's maps with zeros on the mask; bin,
   project and b' against oracle.destriper on w' within the ground file's reordering bound 8 N 2^-53 B
   (B the same expression on absolute values); symmetry under the same bound; two views of one mask
   agree bit for bit; once more under COMAP_POISON=1.  Three problems: the f64 entry form (3000
   offsets x 4 samples, 32 x 32 tiled), the count form (L = 10, one weight per offset, 10 % zeroed)
   and a 4-band stack of the first; each with samples at -1 and at a negative id that wraps onto a
   masked pixel, and a mask that holds the most-hit pixel, a never-hit pixel, a pixel crossed by
   exactly one offset, and a block that empties some offsets and takes only part of others.  (The
   mask also holds the last pixel, which the samples at -1 read: an unbinned sample that reads a
   live pixel makes the reference's operator itself unsymmetric, so the symmetry check needs every
   wrapped read to see 0, as the ground file's cases arrange with a never-hit last row);
2. an all-false mask is the plain solve, bit for bit (x, iterations, every map; one band and four;
   the native and the to_host routes);
3. the converged solve of the seed-0 source case (solve_case(0) plus a Gaussian source of amplitude
   50, sigma 0.6 px at (5.3, 6.4); 13 masked pixels, 5 emptied offsets) against np.linalg.lstsq(A',
   b'), RTOL = 1e-5 (relmax) after removing each vector's mean over the non-empty offsets; x[empty]
   == 0.0 exactly; weight / hits / naive equal the unmasked solve's; the map is the full-weight bin
   of tod - F x_dense;
4. the mask does its job: rms(x - truth) masked / plain < 0.6 (a cap: dense solves give 0.23 at seed
   0 and at most 0.40 over seeds 0 - 5);
5. with the prior: native and eager against np.linalg.solve(A' + T, b') at RTOL with equal iteration
   counts; on the five emptied offsets rms error with / without the prior < 0.85 (a cap: dense solves
   give 0.67 at seed 0, 0.43 - 0.67 over seeds 0 - 5);
6. a 4-band batched masked solve: each band's iteration count, x and map are its own one-band solve's;
7. a split with one label over every offset is the result's own map; the residual sum over all groups
   is NumPy's sum w (tod - F x - m[p])^2 with the full w;
8. set_solve_mask(None) restores test 2's bits; set_solve_mask(mask) on a plain-built destriper equals
   building with the mask;
10. the driver (a FITS mask, the two-pass 'snr' form) and the error table.
(9, the ranks, is test_gpu_destriper_mask_ranks.py.)

Bounds.  Test 1's is the worst-case reordering error of sums of at most N terms (the ground file's
derivation).  Tests 3 and 5 use the project's RTOL: cond(A' + T) = 43 and the CG stops at 1e-14 in rr
/ rr0 (the CPU oracle CG at 1e-14 reaches 7e-7 of lstsq after 98 iterations)."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
import test_gpu_destriper_ground as G  # noqa: E402
import test_gpu_destriper_prior as P  # noqa: E402

pytestmark = pytest.mark.gpu

RTOL = G.RTOL
EPS = G.EPS
NY = NX = 32


# ---------------------------------------------------------------- 1. the view against the definition
def view_case(kind):
    """{'pix', 'tod', 'w', 'L', 'npix', 'mask', ...} of one of test 1's three problems, with the
    properties the docstring lists asserted on the case itself."""
    L = 10 if kind == 'count' else 4
    n = 12000
    NO = n // L
    t = np.arange(n)
    x = (NX - 1) * (0.5 + 0.5 * np.sin(2 * np.pi * t / 517.3))          # permuted_problem's pointing
    y = (NY - 1) * (0.5 + 0.5 * np.sin(2 * np.pi * t / 3011.7 + 1))
    pix = (np.rint(y) * NX + np.rint(x)).astype(np.int64)
    npix = NY * NX
    rng = np.random.default_rng(4)
    nb = 4 if kind == 'bands' else 1
    tod = rng.standard_normal((nb, n))
    if kind == 'count':
        w = np.repeat(0.5 + rng.random(NO), L)[None, :].copy()
        w[0, rng.random(n) < 0.10] = 0.0
    else:
        w = 0.5 + rng.random((nb, n))
    off = t // L
    on = np.ones(n, bool)
    hits = np.bincount(pix, minlength=npix)
    crossing = np.zeros((npix,), np.int64)                               # distinct offsets per pixel
    crossing[:] = np.bincount(np.unique(np.stack([pix, off], 1), axis=0)[:, 0], minlength=npix)
    most, never = int(np.argmax(hits)), int(np.nonzero(hits == 0)[0][0])
    once = int(np.nonzero(crossing == 1)[0][0])
    mask = np.zeros(npix, bool)
    mask[[most, never, once, npix - 1]] = True                           # (npix - 1: what the samples at -1 read)
    by, bx = (10, 12) if kind != 'count' else (8, 10)                    # a block the scan crosses
    side = 3 if kind != 'count' else 7
    blk = np.zeros((NY, NX), bool)
    blk[by:by + side, bx:bx + side] = True
    mask |= blk.reshape(-1)
    # unbinned samples: -1 (reads the last pixel) and a negative id that wraps onto the most-hit pixel
    neg = rng.random(n) < 0.03
    ids = np.where(rng.random(int(neg.sum())) < 0.5, -1, most - npix)
    pix[neg] = ids
    on[neg] = False
    assert np.any(pix == -1) and np.any(pix == most - npix) and mask[most]
    assert hits[never] == 0 and mask[never] and crossing[once] == 1 and mask[once]
    gone = on & mask[np.where(on, pix, 0)]                               # the samples the mask takes
    wm = np.where(gone[None, :], 0.0, w)
    had = (w != 0).reshape(nb, NO, L).any(2)
    left = (wm != 0).reshape(nb, NO, L).any(2)
    empty = had & ~left
    part = left & (gone[None, :] & (w != 0)).reshape(nb, NO, L).any(2)
    assert empty.any(1).all() and part.any(1).all(), (empty.sum(1), part.sum(1))
    return {'kind': kind, 'pix': pix.astype(np.int32), 'tod': tod, 'w': w, 'wm': wm, 'L': L, 'NO': NO, 'npix': npix,
            'nb': nb, 'mask': mask, 'empty': empty}


def build(c, mask='own'):
    from comapreduce_amd.mapmaking.destriper import DeviceDestriper
    m = c['mask'] if isinstance(mask, str) else mask
    one = c['nb'] == 1
    return DeviceDestriper(c['pix'], c['tod'][0] if one else c['tod'], c['w'][0] if one else c['w'], c['L'], c['npix'],
                           map_shape=(NY, NX), solve_mask=m)


def abs_bound(pix, z, w, L, npix):
    """B of A'z: the operator's sums on absolute values, both parts added."""
    from oracle.destriper import bin_offset_map, share_map
    m, h = bin_offset_map(pix, np.abs(z), w, npix)
    m = share_map(m, h)
    return np.sum(np.reshape(w * (np.abs(z) + m[pix]), (z.size // L, L)), axis=1)


def check_view(kind):
    import torch
    from oracle.destriper import bin_offset_map, op_Ax
    c = view_case(kind)
    dd = build(c)
    ops, sops = dd.ops, dd.sops
    nb, NO, L, npix, pix = c['nb'], c['NO'], c['L'], c['npix'], c['pix'].astype(np.int64)
    assert sops is not ops and sops.parent is ops and ops.nb == nb
    assert ops.entry_bytes() == (4 + nb if kind == 'count' else 4 + 8 * nb) == sops.entry_bytes()
    pos = ops.natural(torch.arange(NO, dtype=torch.float64, device=ops.dev).repeat_interleave(nb))
    pos = pos.cpu().numpy().reshape(NO, nb)[:, 0].astype(np.int64)
    assert not np.array_equal(pos, np.arange(NO)) and np.array_equal(np.sort(pos), np.arange(NO))

    def internal(u):                                   # [nb, NO] caller's order -> interleaved internal
        v = np.empty((NO, nb))
        v[pos] = u.T
        return torch.from_numpy(v.reshape(-1)).to(ops.dev)

    def natural(t):                                    # interleaved internal -> [nb, NO]
        return t.cpu().numpy().reshape(NO, nb)[pos].T

    def caller_map(t):                                 # internal (tiled) map -> [nb, npix]
        return dd._untile(t, nb).cpu().numpy().reshape(-1, nb).T

    # h' and nnum' are the parent's maps with zeros on the mask
    (h0, hits0, n0), (h1, hits1, n1) = ops.local_maps(), sops.local_maps()
    for a0, a1 in ((h0, h1), (n0, n1)):
        want = caller_map(a0)
        want[:, c['mask']] = 0.0
        got = caller_map(a1)
        assert np.array_equal(got, want) and not np.any(np.signbit(got[:, c['mask']]))
    assert torch.equal(hits0, hits1)

    def device(o, u):
        ud = internal(u)
        num, q = o.zeros(o.npix * nb), o.zeros(NO * nb)
        o.bin(ud, 0, num)
        o.project(ud, num, h1, q)
        return caller_map(num), natural(q), (num, q)

    rng = np.random.default_rng(3)
    u, v = rng.standard_normal((nb, NO)), rng.standard_normal((nb, NO))
    N = pix.size
    tol = 8 * N * EPS
    (nu, qu, raw_u), (_, qv, _) = device(sops, u), device(sops, v)
    b1 = sops.zeros(NO * nb)
    sops.project(None, n1, h1, b1)
    bdev = natural(b1)
    worst = 0.0
    for b in range(nb):
        wm = c['wm'][b]
        zu, zv = np.repeat(u[b], L), np.repeat(v[b], L)
        num, _ = bin_offset_map(pix, zu, wm, npix)
        bnum, _ = bin_offset_map(pix, np.abs(zu), wm, npix)
        assert np.all(np.abs(nu[b] - num) <= tol * bnum), (kind, b, 'bin')
        Bu, Bv = abs_bound(pix, zu, wm, L, npix), abs_bound(pix, zv, wm, L, npix)
        for name, got, z, bnd in (('u', qu[b], u[b], Bu), ('v', qv[b], v[b], Bv)):
            err = np.abs(got - op_Ax(z, pix, wm, L, npix))
            worst = max(worst, float(np.max(err / np.maximum(tol * bnd, 1e-300))))
            assert np.all(err <= tol * bnd), (kind, b, name)
        err = np.abs(bdev[b] - op_Ax(c['tod'][b], pix, wm, L, npix, extend=False))
        assert np.all(err <= tol * abs_bound(pix, c['tod'][b], wm, L, npix)), (kind, b, 'rhs')
        asym = abs(float(u[b] @ qv[b]) - float(v[b] @ qu[b]))
        assert asym <= tol * (float(np.abs(u[b]) @ Bv) + float(np.abs(v[b]) @ Bu)), (kind, b, asym)
        # an emptied offset has a zero row and b' = 0
        e = c['empty'][b]
        assert np.all(qu[b][e] == 0.0) and np.all(bdev[b][e] == 0.0)
    print(f'{kind}: max |dev - ref| / (8 N eps B) = {worst:.3g}')
    # the mask is felt: A'u is not A u
    _, q_full, _ = device(ops, u)
    assert not np.array_equal(q_full, qu)
    # two views built from one mask agree bit for bit
    twin = ops.masked_view(sops.mask)
    h2, _, n2 = twin.local_maps()
    assert torch.equal(h2, h1) and torch.equal(n2, n1)
    _, _, raw2 = device(twin, u)
    assert torch.equal(raw2[0], raw_u[0]) and torch.equal(raw2[1], raw_u[1])
    b2 = twin.zeros(NO * nb)
    twin.project(None, n2, h2, b2)
    assert torch.equal(b2, b1)
    return True


@pytest.mark.parametrize('kind', ['f64', 'count', 'bands'])
def test_view_against_the_definition(kind):
    assert check_view(kind)


def test_view_under_poison():
    env = dict(os.environ, COMAP_POISON='1')
    code = ('import sys; sys.path[:0] = [%r, %r]; import test_gpu_destriper_mask as T; '
            '[T.check_view(k) for k in ("f64", "count", "bands")]; print("poison ok")'
            % (os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__))))
    r = subprocess.run([sys.executable, '-s', '-c', code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and 'poison ok' in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_parent_outlives_its_view():
    from comapreduce_amd import _native as N
    c = view_case('f64')
    dd = build(c)
    assert N.lib().comap_destripe_destroy(dd.ops.h) == -1             # refused while the view lives
    assert b'view' in N.lib().comap_last_error(dd.ops.ctx)
    with pytest.raises(ValueError, match='view of a view'):
        dd.sops.masked_view(dd.sops.mask)
    res = dd.solve(1e-8, 40)                                            # both handles still work
    assert np.isfinite(res['x'].cpu().numpy()).all()


# ---------------------------------------------------------------- 2. an all-false mask is the plain solve
def results_equal(a, b):
    import torch
    t = lambda v: v.cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)     # noqa: E731
    assert np.array_equal(t(a['x']), t(b['x'])), 'x'
    assert np.array_equal(np.asarray(a['iters']), np.asarray(b['iters'])), (a['iters'], b['iters'])
    assert sorted(a['maps']) == sorted(b['maps'])
    for k in a['maps']:
        assert np.array_equal(t(a['maps'][k]), t(b['maps'][k]), equal_nan=True), k


@pytest.mark.parametrize('kind', ['f64', 'bands'])
def test_all_false_mask_is_the_plain_solve(kind):
    c = view_case(kind)
    plain, masked = build(c, None), build(c, np.zeros(c['npix'], bool))
    assert plain.sops is plain.ops and masked.sops is not masked.ops
    for to_host in (False, True):
        a, b = plain.solve(1e-10, 80, to_host=to_host), masked.solve(1e-10, 80, to_host=to_host)
        assert np.all(np.asarray(a['iters']) > 5)
        results_equal(a, b)
        assert 'solve_mask' not in a and b['solve_mask']['pixels'] == 0
        assert np.all(np.asarray(b['solve_mask']['samples']) == 0)


# ---------------------------------------------------------------- 3 - 5. the seed-0 source case
def source_case(seed=0):
    """solve_case(seed) plus a Gaussian source (amplitude 50, sigma 0.6 px) at x = 5.3, y = 6.4 and the
    mask of the pixels within 2 px of it."""
    c = P.solve_case(seed)
    t = np.arange(c['pix'].size)
    x = 11 * (0.5 + 0.5 * np.sin(2 * np.pi * t / 777.3))                # solve_case's own scan
    y = 11 * (0.5 + 0.5 * np.sin(2 * np.pi * t / 5113.7 + 1))
    assert np.array_equal((np.rint(y) * 12 + np.rint(x)).astype(np.int32), c['pix'])
    c['tod'] = c['tod'] + 50.0 * np.exp(-((x - 5.3) ** 2 + (y - 6.4) ** 2) / (2 * 0.6 ** 2))
    py, px = np.divmod(np.arange(144), 12)
    c['mask'] = (px - 5.3) ** 2 + (py - 6.4) ** 2 <= 4.0
    c['wm'] = np.where(c['mask'][c['pix']], 0.0, c['w'])
    c['empty'] = c['wm'].reshape(c['NO'], c['L']).sum(axis=1) == 0
    assert int(c['mask'].sum()) == 13 and int(c['empty'].sum()) == 5
    return c


def dense_system_w(c, w):
    """test_gpu_destriper_prior.dense_system generalised to weights: (A, b) of F^T W Z F x = F^T W Z d."""
    L, NO, npix, pix = c['L'], c['NO'], c['npix'], c['pix'].astype(np.int64)
    off = np.arange(pix.size) // L
    h = np.bincount(pix, weights=w, minlength=npix)

    def FtZ(z):
        m = np.bincount(pix, weights=w * z, minlength=npix)
        m = np.where(h != 0, m / np.where(h != 0, h, 1.0), m)
        return np.bincount(off, weights=w * (z - m[pix]), minlength=NO)

    A = np.stack([FtZ(e[off]) for e in np.eye(NO)], axis=1)
    return A, FtZ(c['tod'])


@pytest.fixture(scope='module')
def source():
    c = source_case(0)
    A0, b0 = P.dense_system(c)
    A1, b1 = dense_system_w(c, np.ones_like(c['w']))
    assert np.array_equal(A0, A1) and np.array_equal(b0, b1)          # the generalisation restates it
    A, b = dense_system_w(c, c['wm'])
    return c, A, b, np.linalg.lstsq(A, b, rcond=1e-10)[0]


def solve_source(c, mask, prior=None, mode=None, **kw):
    from comapreduce_amd.mapmaking.destriper import DeviceDestriper
    if mode is not None:
        os.environ['COMAP_DS_PRIOR_SOLVE'] = mode
    try:
        dd = DeviceDestriper(c['pix'], c['tod'], c['w'], c['L'], c['npix'], map_shape=(12, 12), prior=prior,
                             solve_mask=mask, **kw)
        res = dd.solve(1e-14, 300)
    finally:
        os.environ.pop('COMAP_DS_PRIOR_SOLVE', None)
    res['x'] = res['x'].cpu().numpy()
    res['maps'] = {k: v.cpu().numpy() for k, v in res['maps'].items()}
    return res


def centred(x, keep):
    return x - x[keep].mean()


def rms_truth(c, x):
    d = x - c['truth']
    return float(np.std(d - d.mean()))


def test_converged_solve_matches_lstsq(source):
    c, A, b, want = source
    keep = ~c['empty']
    assert np.all(A[c['empty']] == 0) and np.all(b[c['empty']] == 0)
    res = solve_source(c, c['mask'])
    plain = solve_source(c, None)
    x = res['x']
    e = G.relmax(centred(x, keep)[keep], centred(want, keep)[keep])
    print(f'masked solve vs lstsq: relmax {e:.3g} after {res["iters"]} iterations')
    assert e <= RTOL and 5 < res['iters'] < 300
    assert np.all(x[c['empty']] == 0.0) and not np.any(np.signbit(x[c['empty']]))
    for k in ('weight', 'hits', 'naive'):
        assert np.array_equal(res['maps'][k], plain['maps'][k], equal_nan=True), k
    pix = c['pix'].astype(np.int64)
    h = np.bincount(pix, weights=c['w'], minlength=c['npix'])
    m = np.bincount(pix, weights=c['w'] * (c['tod'] - np.repeat(want, c['L'])), minlength=c['npix'])
    m = np.where(h != 0, m / np.where(h != 0, h, 1.0), m)
    # (the CG starts at x = 0 and b' has no null-space part, so x shares the dense solution's level)
    em = G.relmax(res['maps']['map'], m)
    print(f'map vs the full-weight bin of tod - F x_dense: relmax {em:.3g}')
    assert em <= RTOL
    assert res['solve_mask'] == {'pixels': 13, 'samples': int((c['wm'] == 0).sum()), 'empty_offsets': 5}
    assert 'solve_mask' not in plain


def test_the_mask_does_its_job(source):
    c, _, _, _ = source
    masked, plain = solve_source(c, c['mask']), solve_source(c, None)
    ratio = rms_truth(c, masked['x']) / rms_truth(c, plain['x'])
    print(f'rms(x - truth): masked {rms_truth(c, masked["x"]):.4g}, plain {rms_truth(c, plain["x"]):.4g}, '
          f'ratio {ratio:.3g}')
    assert ratio < 0.6


def test_with_the_prior(source):
    c, A, b, _ = source
    gid, stencil = P.prior_of(1)
    T = P.dense_T(gid, stencil)
    want = np.linalg.solve(A + T, b)
    native = solve_source(c, c['mask'], (gid, stencil), 'native')
    eager = solve_source(c, c['mask'], (gid, stencil), 'eager')
    en, ee = G.relmax(native['x'], want), G.relmax(eager['x'], want)
    print(f'masked + prior vs dense: native {en:.3g} ({native["iters"]} it), eager {ee:.3g} ({eager["iters"]} it)')
    assert en <= RTOL and ee <= RTOL and native['iters'] == eager['iters'] and 5 < native['iters'] < 300
    # both routes bin the maps from the full problem
    plain = solve_source(c, None)
    for r in (native, eager):
        assert np.array_equal(r['maps']['weight'], plain['maps']['weight'])
        assert np.array_equal(r['maps']['naive'], plain['maps']['naive'], equal_nan=True)
    assert G.relmax(native['maps']['map'], eager['maps']['map']) <= RTOL
    # the prior carries the emptied offsets across from their neighbours
    without = solve_source(c, c['mask'])
    e = c['empty']
    err = lambda x: float(np.sqrt(np.mean((x - c['truth'])[e] ** 2)))      # noqa: E731
    ratio = err(native['x']) / err(without['x'])
    print(f'rms error on the 5 emptied offsets: prior {err(native["x"]):.4g}, none {err(without["x"]):.4g}, '
          f'ratio {ratio:.3g}')
    assert ratio < 0.85


# ---------------------------------------------------------------- 6. bands
def test_bands_are_their_own_solves():
    from comapreduce_amd.mapmaking.destriper import DeviceDestriper
    c = view_case('bands')
    batched = build(c).solve(1e-10, 200)
    for b in range(4):
        one = DeviceDestriper(c['pix'], c['tod'][b], c['w'][b], c['L'], c['npix'], map_shape=(NY, NX),
                              solve_mask=c['mask']).solve(1e-10, 200)
        assert int(batched['iters'][b]) == int(one['iters']) and 5 < int(one['iters']) < 200, (b, batched['iters'])
        assert G.relmax(batched['x'][b].cpu().numpy(), one['x'].cpu().numpy()) <= RTOL
        assert G.relmax(batched['maps']['map'][b].cpu().numpy(), one['maps']['map'].cpu().numpy()) <= RTOL
        assert int(batched['solve_mask']['empty_offsets'][b]) == int(one['solve_mask']['empty_offsets']) > 0
        assert int(batched['solve_mask']['samples'][b]) == int(one['solve_mask']['samples']) > 0


# ---------------------------------------------------------------- 7. splits and residuals
def test_splits_and_residuals_use_the_full_weights(source):
    c, _, _, _ = source
    NO, L = c['NO'], c['L']
    feed, obs = np.full(NO * L, 3), np.full(NO * L, 41)
    res = solve_source(c, c['mask'], split=(np.zeros(NO, np.int32), 1), residuals=True, residual_groups=(feed, obs))
    sp = {k: v.cpu().numpy() for k, v in res['splits'].items()}
    assert sp['map'].shape == (1, c['npix'])
    assert G.relmax(sp['map'][0], res['maps']['map']) <= RTOL
    assert np.array_equal(sp['weight'][0], res['maps']['weight'])
    pix = c['pix'].astype(np.int64)
    r = c['tod'] - np.repeat(res['x'], L) - res['maps']['map'][pix]
    want = float(np.sum(c['w'] * r * r))
    got = float(res['residuals']['sum'].cpu().numpy().sum())
    print(f'residual sum: device {got:.10g}, NumPy {want:.10g}')
    assert abs(got - want) <= RTOL * want
    assert int(res['residuals']['count'].cpu().numpy().sum()) == NO * L     # the masked samples count too


# ---------------------------------------------------------------- 8. re-masking
def test_re_masking():
    c = view_case('f64')
    plain = build(c, None)
    want_plain = plain.solve(1e-10, 80)
    built = build(c)
    want_masked = built.solve(1e-10, 80)
    assert not np.array_equal(want_masked['x'].cpu().numpy(), want_plain['x'].cpu().numpy())
    built.set_solve_mask(None)
    assert built.sops is built.ops
    back = built.solve(1e-10, 80)
    results_equal(back, want_plain)
    assert 'solve_mask' not in back
    parent = plain.ops
    plain.set_solve_mask(c['mask'])
    assert plain.ops is parent and plain.sops is not parent             # only the view was built
    again = plain.solve(1e-10, 80)
    results_equal(again, want_masked)
    assert again['solve_mask'] == want_masked['solve_mask']


def test_re_masking_keeps_the_prior(source):
    from comapreduce_amd.mapmaking.destriper import DeviceDestriper
    c, _, _, _ = source
    prior = P.prior_of(1)
    dd = DeviceDestriper(c['pix'], c['tod'], c['w'], c['L'], c['npix'], map_shape=(12, 12), prior=prior)
    first = dd.pops
    dd.set_solve_mask(c['mask'])
    assert dd.pops is not first and dd.pops.ops is dd.sops and dd.sops is not dd.ops
    a = dd.solve(1e-14, 300)
    b = solve_source(c, c['mask'], prior)
    assert np.array_equal(a['x'].cpu().numpy(), b['x']) and int(a['iters']) == int(b['iters'])


# ---------------------------------------------------------------- 10. the driver and the error table
def driver_kw(cc, store):
    m = cc.CASES['car']['map']
    return dict(offset_length=50, prefix='t', feeds=cc.FEEDS, nxpix=m['nxpix'], nypix=m['nypix'], crval=m['crval'],
                crpix=m['crpix'], ctype=m['ctype'], cdelt=m['cdelt'], use_gain_filter=True, calibration=False,
                threshold=1e-6, niter=50, store=store)


def test_driver_fits_mask(tmp_path):
    import comapdata_case as cc
    from comapreduce_amd.mapmaking.fits import read_image_hdus, write_image_hdus
    from comapreduce_amd.mapmaking.run_destriper import main
    store, names = cc.store()
    names = names[:2]                                   # Field00 files (non-calibrator mode)
    kw = driver_kw(cc, store)
    ny, nx = kw['nypix'], kw['nxpix']
    plain = main(names, output_dir=str(tmp_path / 'plain'), bands=(0, 1), **kw)
    hits = np.reshape(plain[0]['All']['hits'], (ny, nx))
    mask = np.zeros((ny, nx))
    yy, xx = np.unravel_index(int(np.argmax(hits)), hits.shape)
    mask[max(yy - 1, 0):yy + 2, max(xx - 1, 0):xx + 2] = 1.0
    write_image_hdus(str(tmp_path / 'mask.fits'), [(None, mask)])
    masked = main(names, output_dir=str(tmp_path / 'masked'), bands=(0, 1), solve_mask=str(tmp_path / 'mask.fits'), **kw)
    files = sorted(os.listdir(tmp_path / 'plain'))
    assert files and files == sorted(os.listdir(tmp_path / 'masked'))
    for f in files:
        a, b = read_image_hdus(str(tmp_path / 'plain' / f)), read_image_hdus(str(tmp_path / 'masked' / f))
        assert len(b) == len(a) + 1 and b[-1][0]['EXTNAME'] == 'SolveMask'
        assert np.array_equal(b[-1][1], mask)
        for (ha, da), (hb, db) in zip(a[1:], b[1:-1]):               # Naive, Noise, Hits: as without the mask
            assert ha == hb and np.array_equal(da, db, equal_nan=True)
        fin = np.isfinite(a[0][1])
        assert np.array_equal(np.isfinite(b[0][1]), fin) and not np.array_equal(a[0][1][fin], b[0][1][fin])
    for band in (0, 1):
        info = masked[band]['solve_mask']
        assert info['pixels'] == int(mask.sum()) and info['samples'] > 0 and 'solve_mask' not in plain[band]
    # the per-band loop writes the same files
    loop = main(names, output_dir=str(tmp_path / 'loop'), bands=(0, 1), solve_mask=str(tmp_path / 'mask.fits'),
                batch_bands=False, **kw)
    assert files == sorted(os.listdir(tmp_path / 'loop'))
    for f in files:
        a, b = read_image_hdus(str(tmp_path / 'masked' / f)), read_image_hdus(str(tmp_path / 'loop' / f))
        assert len(a) == len(b) and np.array_equal(a[-1][1], b[-1][1])
        for (_, da), (_, db) in zip(a[1:], b[1:]):
            assert np.array_equal(da, db, equal_nan=True)
    assert loop[0]['solve_mask']['pixels'] == int(mask.sum())
    # a NaN or another shape in the file
    bad = mask.copy()
    bad[0, 0] = np.nan
    write_image_hdus(str(tmp_path / 'nan.fits'), [(None, bad)])
    write_image_hdus(str(tmp_path / 'small.fits'), [(None, mask[:-1])])
    for f in ('nan.fits', 'small.fits'):
        with pytest.raises(ValueError, match='solve_mask'):
            main(names, output_dir=str(tmp_path / 'bad'), bands=(0,), solve_mask=str(tmp_path / f), **kw)
    with pytest.raises(NotImplementedError):
        main(names, output_dir=str(tmp_path / 'bad'), bands=(0,), solve_mask=str(tmp_path / 'mask.fits'),
             **dict(kw, healpix=True))


def noise_field(cc, store, names):
    """The store's Level-2 tod replaced by white noise of sigma 5e-3 inside the scans (exact zeros kept:
    the masked run), so that the first-pass map holds noise only -- the condition of the 'snr' test's
    input.  The prep's weight is 1 / auto_rms^2 of the WHOLE file row, the samples outside the scans
    included (zeros in the synthetic files, which would make the claimed sigma 0.55 of the true one and
    5 claimed sigma a 2.7 sigma cut); noise of 2.5 times the sigma there makes the claim 1.2 times the
    truth, i.e. the cut conservative.  Those samples are never mapped."""
    from comapreduce_amd.mapmaking import comapdata as COMAPData
    rng = np.random.default_rng(5)
    for fn in names:
        d = store[fn][0]
        tod = np.asarray(d['averaged_tod/tod'])
        inscan = np.zeros(tod.shape[-1], bool)
        for s, e in d['averaged_tod/scan_edges']:
            inscan[s:e] = True
        new = np.where(tod != 0, 5e-3 * rng.standard_normal(tod.shape), 0.0)
        new[..., ~inscan] = 12.5e-3 * rng.standard_normal(new[..., ~inscan].shape)
        d['averaged_tod/tod'] = new
        claimed = COMAPData.auto_rms(new[1, 0])
        assert 5.5e-3 < claimed < 6.5e-3, claimed


def inject_source(store, names, kw, pixel, amp):
    """Add ``amp`` to every non-zero Level-2 sample (all feeds and bands) that points at map pixel
    ``pixel``; returns their number."""
    from comapreduce_amd.mapmaking import comapdata as COMAPData
    info = COMAPData.map_info_from(kw['crval'], kw['cdelt'], kw['crpix'], kw['ctype'], kw['nxpix'], kw['nypix'])
    n = 0
    for fn in names:
        d = store[fn][0]
        ra, dec = d['spectrometer/pixel_pointing/pixel_ra'], d['spectrometer/pixel_pointing/pixel_dec']
        pix = np.asarray(COMAPData.transform_to_1d(np.ravel(ra), np.ravel(dec), info['wcs'], kw['nxpix'],
                                                   kw['nypix'])).reshape(ra.shape)
        tod = np.array(d['averaged_tod/tod'])
        for f in range(tod.shape[0]):
            at = (pix[f] == pixel)[None, :] & (tod[f] != 0)
            tod[f][at] += amp
            n += int(at[0].sum())
        d['averaged_tod/tod'] = tod
    return n


def test_driver_snr_mask(tmp_path):
    """A noise-only field with one injected source, 50 sigma in its pixel: the two-pass form masks it
    and at most 2 % of the other hit pixels (a condition of the input, asserted), and yields the maps
    of that mask passed as a file."""
    import comapdata_case as cc
    from comapreduce_amd.mapmaking.fits import write_image_hdus
    from comapreduce_amd.mapmaking.run_destriper import main
    store, names = cc.store()
    names = names[:2]
    kw = driver_kw(cc, store)
    ny, nx = kw['nypix'], kw['nxpix']
    noise_field(cc, store, names)
    plain = main(names, output_dir=str(tmp_path / 'plain'), bands=(0,), **kw)[0]['All']
    w = np.reshape(plain['weight'], (ny, nx))
    hit = w > 0
    # the source's pixel: a well-hit pixel the scans cross quickly, nearest the middle of the hit region (the
    # most-hit pixels are turn-rounds, where one offset holds many of the pixel's samples)
    hits = np.reshape(plain['hits'], (ny, nx))
    ys, xs = np.nonzero(hit)
    good = hits[ys, xs] >= np.median(hits[ys, xs])
    k = np.argmin(np.where(good, (ys - ys.mean()) ** 2 + (xs - xs.mean()) ** 2, np.inf))
    yy, xx = int(ys[k]), int(xs[k])
    assert 0 < yy < ny - 1 and 0 < xx < nx - 1
    assert inject_source(store, names, kw, yy * nx + xx, 50.0 / np.sqrt(w[yy, xx])) > 0
    snr = main(names, output_dir=str(tmp_path / 'snr'), bands=(0,), solve_mask=('snr', 5, 1), **kw)[0]
    found = snr['solve_mask']['mask'].reshape(ny, nx) != 0
    cross = np.zeros((ny, nx), bool)
    cross[yy - 1:yy + 2, xx] = True
    cross[yy, xx - 1:xx + 2] = True
    assert np.all(found[cross])                                         # the source, grown once
    others = found & ~cross
    print(f'snr mask: {int(found.sum())} pixels, {int(others.sum())} away from the source, of {int(hit.sum())} hit')
    assert others.sum() <= 0.02 * (hit & ~cross).sum(), (int(others.sum()), int(hit.sum()))
    write_image_hdus(str(tmp_path / 'found.fits'), [(None, found.astype(float))])
    filed = main(names, output_dir=str(tmp_path / 'filed'), bands=(0,), solve_mask=str(tmp_path / 'found.fits'),
                 batch_bands=False, **kw)[0]
    for k in ('map', 'naive', 'weight', 'hits'):
        assert np.array_equal(snr['All'][k], filed['All'][k], equal_nan=True), k
    assert snr['solve_mask']['pixels'] == filed['solve_mask']['pixels'] == int(found.sum())
    assert sorted(os.listdir(tmp_path / 'snr')) == sorted(os.listdir(tmp_path / 'filed'))
    assert snr['solve_mask']['samples'] > 0


def test_error_table():
    from comapreduce_amd.mapmaking.destriper import DeviceDestriper, run_destriper, run_destriper_bands
    c = source_case(0)
    args = (c['pix'], c['tod'], c['w'], c['L'], c['npix'])
    n = c['pix'].size
    with pytest.raises(NotImplementedError, match='ground'):
        DeviceDestriper(*args, solve_mask=c['mask'], ground=(np.zeros(n), np.zeros(n), np.zeros(n)))
    with pytest.raises(NotImplementedError, match='residual_cut'):
        DeviceDestriper(*args, solve_mask=c['mask'], residual_groups=(np.zeros(n), np.zeros(n)), residual_cut=2.0)
    for bad in (c['mask'][:-1], np.zeros((2, 2, 36), bool), c['mask'].reshape(12, 12)):
        with pytest.raises(ValueError, match='solve mask'):
            DeviceDestriper(*args, solve_mask=bad)                      # (2-D without map_shape)
    with pytest.raises(ValueError, match='solve mask'):
        DeviceDestriper(*args, map_shape=(12, 12), solve_mask=np.zeros((9, 16), bool))
    nan = c['mask'].astype(float)
    nan[3] = np.nan
    with pytest.raises(ValueError, match='non-finite'):
        DeviceDestriper(*args, solve_mask=nan)
    edges = np.arange(c['npix'])
    with pytest.raises(NotImplementedError):
        run_destriper(c['pix'], c['tod'], c['w'], c['L'], edges, solve_mask=c['mask'], healpix=True)
    with pytest.raises(NotImplementedError):
        run_destriper_bands(c['pix'], np.stack([c['tod']] * 2), np.stack([c['w']] * 2), c['L'], edges,
                            solve_mask=('snr', 5))
    # the forms that work: uint8 / float flags, 2-D with map_shape; and through run_destriper
    a = DeviceDestriper(*args, map_shape=(12, 12), solve_mask=c['mask'].reshape(12, 12).astype(np.uint8)).solve(1e-10, 99)
    b = DeviceDestriper(*args, map_shape=(12, 12), solve_mask=c['mask'].astype(float)).solve(1e-10, 99)
    assert np.array_equal(a['x'].cpu().numpy(), b['x'].cpu().numpy())
    r = run_destriper(c['pix'], c['tod'], c['w'], c['L'], edges, threshold=1e-10, niter=99, map_shape=(12, 12),
                      solve_mask=c['mask'])
    assert r['solve_mask']['pixels'] == 13 and np.array_equal(r['solve_mask']['mask'] != 0, c['mask'])
    assert np.array_equal(r['All']['map'], a['maps']['map'].cpu().numpy(), equal_nan=True)
