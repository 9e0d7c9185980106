"""Residual chi-squared per offset and per (observation, feed) group: the device pass
comap_destripe_residuals and its path up through DeviceOps.residuals, DeviceDestriper(residuals=,
residual_cut=), run_destriper and run_destriper_bands, against the NumPy restatement below.  The
sums run in the lane-tree order (destriper.lane_tree_sum), every operation rounded on its own, so
sums and counts must be equal bit for bit (array_equal), not close, on the DEVICE's own x and map.

Inputs: the cases of test_gpu_destriper_ground.py (A: L = 10, 1150 samples, 144 pixels, negative
pixel ids and zero weights, one (observation, feed) absent; B: 60 000 samples, L = 50) and small
cases built here for the offset lengths that exercise the lane loop."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_destriper_ground import CASE_A, CASE_B, make_case, relmax  # noqa: E402,F401

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------- the restatement
def restate(pix, tod, w, x, m, L, gid=None, G=0, keep=None):
    """One band: (off_sum [N/L], off_cnt, grp_sum [G], grp_cnt).  A sample is counted when
    pix >= 0, w > 0 and its offset is kept; term = (w r) r, r = (tod - x[o]) - m[pix]; an uncounted
    sample's term is +0.0; sums by lane_tree_sum, a group's over its offsets in increasing order."""
    from comapreduce_amd.mapmaking.destriper import lane_tree_sum
    pix = np.asarray(pix, np.int64)
    NO = pix.size // L
    counted = (pix >= 0) & (w > 0)
    if keep is not None:
        counted &= np.repeat(np.asarray(keep) != 0, L)
    r = (tod - np.repeat(x, L)) - m[np.where(pix >= 0, pix, 0)]
    term = np.where(counted, (w * r) * r, 0.0).reshape(NO, L)
    off_sum = np.array([lane_tree_sum(t) for t in term]).reshape(NO)
    off_cnt = counted.reshape(NO, L).sum(axis=1)
    if gid is None:
        return off_sum, off_cnt, None, None
    gid = np.asarray(gid)
    grp_sum = np.array([lane_tree_sum(off_sum[gid == g]) for g in range(G)])
    grp_cnt = np.array([off_cnt[gid == g].sum() for g in range(G)], np.int64)
    return off_sum, off_cnt, grp_sum, grp_cnt


def raw_call(pix, tod, w, x, m, gid, G, L, npix, nb=1, keep=None, null=()):
    """comap_destripe_residuals itself on host inputs (tod / w [nb, N], x [N/L, nb], m [npix, nb]):
    (rc, (off_sum [N/L, nb], off_cnt, grp_sum [G, nb], grp_cnt), the error text).  null: names of
    arguments passed as NULL."""
    import torch
    from comapreduce_amd import _native as N
    dev = torch.device('cuda', N.current_device())
    c = N.ctx()
    N.bind_stream(c, dev)

    def t(a, dt):
        return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(device=dev, dtype=dt).contiguous()
    NO = int(np.size(pix)) // L if np.size(pix) % L == 0 else int(np.size(pix)) // L + 1
    a = {'pix': t(pix, torch.int32), 'tod': t(tod, torch.float64), 'w': t(w, torch.float64), 'keep': t(keep, torch.uint8),
         'x': t(x, torch.float64), 'map': t(m, torch.float64), 'group': t(gid, torch.int32),
         'off_sum': N.device_empty(NO * nb, torch.float64, dev), 'off_cnt': N.device_empty(NO * nb, torch.int32, dev),
         'grp_sum': N.device_empty(max(G, 1) * nb, torch.float64, dev),
         'grp_cnt': N.device_empty(max(G, 1) * nb, torch.int64, dev)}
    p = {k: (None if v is None or k in null else N.dptr(v)) for k, v in a.items()}
    rc = N.lib().comap_destripe_residuals(c, p['pix'], p['tod'], p['w'], p['keep'], p['x'], p['map'], p['group'], G,
                                          int(np.size(pix)), L, npix, nb, p['off_sum'], p['off_cnt'], p['grp_sum'],
                                          p['grp_cnt'])
    torch.cuda.synchronize()
    msg = N.lib().comap_last_error(c).decode()
    out = (a['off_sum'].cpu().numpy().reshape(NO, nb), a['off_cnt'].cpu().numpy().reshape(NO, nb),
           a['grp_sum'].cpu().numpy().reshape(-1, nb), a['grp_cnt'].cpu().numpy().reshape(-1, nb))
    return rc, out, msg


def same(got, want, what):
    """array_equal on every table, the band axis last in ``got``."""
    for g, w_, k in zip(got, want, ('off_sum', 'off_cnt', 'grp_sum', 'grp_cnt')):
        if w_ is not None:
            assert np.array_equal(g, w_), (what, k, int(np.sum(g != w_)))


def groups_of(case):
    from comapreduce_amd.mapmaking.destriper import ground_groups
    gid, uobs, ufeed = ground_groups(case['feed'], case['obs'], case['L'])
    return gid, int(uobs.size * ufeed.size)


# ---------------------------------------------------------------- 1. the C call alone
def check_c_call():
    """Case A through the C entry point alone; also run in a child process under COMAP_POISON=1
    (the variable is read once per process)."""
    case = make_case(**CASE_A)
    L, npix, pix = case['L'], case['npix'], case['pix']
    assert L == 10 and pix.size == 1150 and npix == 144
    assert {-1, -5} <= set(pix.tolist()) and 0.02 < np.mean(case['w'] == 0) < 0.09
    gid, G0 = groups_of(case)
    assert G0 == 6 and np.sum(gid == 4) == 0                  # the absent (observation, feed)
    gid = gid.copy()
    gid[[7, 60]] = -1                                         # two offsets in no group
    rng = np.random.default_rng(2)
    x, m = rng.standard_normal(gid.size), rng.standard_normal(npix)
    args = (pix, case['tod'][None], case['w'][None], x[:, None], m[:, None])
    for G in (G0, G0 + 1):                                    # G0 + 1: one more group that owns no offset
        want = restate(pix, case['tod'], case['w'], x, m, L, gid, G)
        rc, got, msg = raw_call(*args, gid, G, L, npix)
        assert rc == 0, msg
        same([v[:, 0] for v in got], want, G)
        assert want[3][4] == 0 and got[2][4, 0] == 0.0 and np.all(want[3][[0, 1, 2, 3, 5]] > 0)
        if G > G0:
            assert got[2][G0, 0] == 0.0 and got[3][G0, 0] == 0 and not np.signbit(got[2][G0, 0])
        assert want[1].sum() > want[3].sum() > 0              # the two unlabelled offsets hold counted samples
        rc, again, _ = raw_call(*args, gid, G, L, npix)
        assert rc == 0 and all(a.tobytes() == b.tobytes() for a, b in zip(got, again))
    # no group stage: NULL labels and 0 groups, the group outputs may be NULL
    rc, got, msg = raw_call(*args, None, 0, L, npix, null=('grp_sum', 'grp_cnt'))
    assert rc == 0, msg
    same([v[:, 0] for v in got[:2]], want[:2], 'no groups')
    # argument and range errors
    bad = pix.copy()
    bad[17] = npix
    assert raw_call(bad, *args[1:], gid, G0, L, npix)[0] == -3
    bad[17] = -npix - 1
    assert raw_call(bad, *args[1:], gid, G0, L, npix)[0] == -3
    for wrong in (G0, -2):
        lb = gid.copy()
        lb[5] = wrong
        rc, _, msg = raw_call(*args, lb, G0, L, npix)
        assert rc == -4 and 'label' in msg
    for name in ('off_sum', 'off_cnt', 'grp_sum', 'grp_cnt', 'map', 'x'):
        assert raw_call(*args, gid, G0, L, npix, null=(name,))[0] == -1, name
    n1 = pix.size - 3                                         # N % L != 0 (the buffers hold the whole offsets)
    assert raw_call(pix[:n1], case['tod'][None, :n1], case['w'][None, :n1], x[:, None], m[:, None], gid, G0, L,
                    npix)[0] == -1
    assert raw_call(*args, gid, G0, L, npix, nb=3)[0] == -1   # (refused before any buffer is touched)
    check_degenerate_segments()


def check_degenerate_segments():
    """The group stage's segment counts at their smallest (L = 10, 7 pixels, one band, one group):
    only the sentinel's segment (every offset labelled -1), exactly one live segment, no counted
    sample at all (every pixel id -2), and a single offset."""
    L, npix = 10, 7
    rng = np.random.default_rng(11)
    for what, NO, pix, label in (('all labelled -1', 3, None, -1), ('one pixel', 3, 4, 0), ('every pixel -2', 3, -2, 0),
                                 ('one offset', 1, None, 0)):
        n = NO * L
        p = rng.integers(0, npix, n).astype(np.int32) if pix is None else np.full(n, pix, np.int32)
        tod, w, x, m = rng.standard_normal(n), rng.uniform(0.5, 2.0, n), rng.standard_normal(NO), rng.standard_normal(npix)
        gid = np.full(NO, label, np.int32)
        want = restate(p, tod, w, x, m, L, gid, 1)
        rc, got, msg = raw_call(p, tod[None], w[None], x[:, None], m[:, None], gid, 1, L, npix)
        assert rc == 0, (what, msg)
        same([v[:, 0] for v in got], want, what)
        if label < 0:
            assert got[2][0, 0] == 0.0 and not np.signbit(got[2][0, 0]) and got[3][0, 0] == 0, what
            assert got[1].sum() == n and np.all(got[0] > 0), what
        elif pix == -2:
            assert not got[0].any() and not got[1].any() and not got[2].any() and not got[3].any(), what
        else:
            assert got[3][0, 0] == n and got[2][0, 0] > 0, what


def test_c_call_alone():
    check_c_call()


def test_c_call_alone_under_poison():
    env = dict(os.environ, COMAP_POISON='1')
    code = ('import sys; sys.path[:0] = [%r, %r]; import test_gpu_residuals as T; T.check_c_call(); print("poison ok")'
            % (os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__))))
    r = subprocess.run([sys.executable, '-s', '-c', code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and 'poison ok' in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ---------------------------------------------------------------- 2. offset lengths
@pytest.mark.parametrize('L', [1, 10, 64, 65, 250])
def test_offset_lengths_of_the_lane_loop(L):
    """L < 64: a ragged single round (several offsets' loads in flight per wave; 71 offsets is no
    multiple of that number); 64: exactly one round; 65 and 250: several rounds with a ragged tail.
    One group of 70 offsets (its sum wraps past 64 lanes) and one of exactly 1 offset."""
    rng = np.random.default_rng(300 + L)
    NO, npix = 71, 37
    n = NO * L
    pix = rng.integers(0, npix, n).astype(np.int32)
    pix[rng.random(n) < 0.1] = -3
    w = 0.5 + rng.random(n)
    w[rng.random(n) < 0.1] = 0.0
    tod, x, m = rng.standard_normal(n), rng.standard_normal(NO), rng.standard_normal(npix)
    gid = np.array([0] * 70 + [1], np.int32)
    want = restate(pix, tod, w, x, m, L, gid, 2)
    rc, got, msg = raw_call(pix, tod[None], w[None], x[:, None], m[:, None], gid, 2, L, npix)
    assert rc == 0, msg
    same([v[:, 0] for v in got], want, L)
    assert want[3][0] > 0 and want[2][1] == want[0][70]


# ---------------------------------------------------------------- 3. bands
@pytest.mark.parametrize('nb', [2, 3, 4])
def test_bands_with_their_own_keep(nb):
    """Case B's pointing as nb bands with band-specific tod, weights and keep masks (the split
    tests' case).  2 and 4 bands: the C call, with the dropped offsets' weights left non-zero, so
    only keep leaves them out; 3 bands: DeviceOps.residuals, which pads to 4 (the library's own
    convention there: a dropped offset has zero weights)."""
    import torch
    import test_gpu_split_maps as S
    from comapreduce_amd.mapmaking.destriper import DeviceOps
    case, tod, w, keep = S.case_b_bands(nb)
    L, npix, pix = case['L'], case['npix'], case['pix']
    gid, G = groups_of(case)
    rng = np.random.default_rng(70 + nb)
    NO = pix.size // L
    x, m = rng.standard_normal((nb, NO)), rng.standard_normal((nb, npix))
    if nb == 3:
        ops = DeviceOps(pix, tod, w, L, npix, keep=keep)
        assert ops.nb == 4
        mi = torch.zeros((npix, 4), dtype=torch.float64, device=ops.dev)
        mi[:, :3] = torch.from_numpy(np.ascontiguousarray(m.T)).to(ops.dev)
        out = ops.residuals(S.interleaved(ops, x), mi.reshape(-1), torch.from_numpy(gid).to(ops.dev), G)
        got = [v.cpu().numpy().reshape(-1, 4) for v in out]
        assert all(np.all(v[:, 3] == 0) for v in got)         # the padded band: nothing counted
    else:
        w = np.where(w > 0, w, np.where(case['w'] > 0, 0.7, 0.0)[None, :])     # dropped offsets: weights back
        assert np.all((w.reshape(nb, NO, L) > 0).any(axis=2))
        rc, got, msg = raw_call(pix, tod, w, x.T, m.T, gid, G, L, npix, nb=nb, keep=keep)
        assert rc == 0, msg
    for b in range(nb):
        want = restate(pix, tod[b], w[b], x[b], m[b], L, gid, G, keep[b])
        same([v[:, b] for v in got], want, (nb, b))
        assert np.all(want[1][keep[b] == 0] == 0) and np.sum(keep[b] == 0) > 60
    only = (keep[0] == 0) & (keep[1] != 0)                      # dropped in band 0 only
    assert only.sum() > 0 and np.all(got[1][only, 0] == 0) and np.all(got[1][only, 1] > 0)


# ---------------------------------------------------------------- 4. through DeviceDestriper
def check_tables(res, pix, tod, w, L, gid, G, keep=None):
    """res['residuals'] against the restatement on the caller-order map and x of the same solve;
    returns the tables as host arrays."""
    r = {k: np.asarray(v.cpu().numpy() if hasattr(v, 'cpu') else v) for k, v in res['residuals'].items()}
    x2 = np.atleast_2d(res['x'].cpu().numpy())
    m2 = np.atleast_2d(np.asarray(res['maps']['map'].cpu().numpy() if hasattr(res['maps']['map'], 'cpu')
                                  else res['maps']['map']))
    tod2, w2 = np.atleast_2d(tod), np.atleast_2d(w)
    for b in range(tod2.shape[0]):
        want = restate(pix, tod2[b], w2[b], x2[b], m2[b], L, gid, G, None if keep is None else keep[b])
        got = [np.atleast_2d(r[k])[b] for k in ('offset_sum', 'offset_count', 'sum', 'count')]
        same(got, want, b)
        chi2 = np.where(want[3] > 0, want[2] / np.where(want[3] > 0, want[3], 1), 0.0)
        assert np.array_equal(np.atleast_2d(r['chi2'])[b], chi2)
    return r


@pytest.mark.parametrize('tile', ['tiled', 'row_major'])
def test_device_destriper_tables(tile, monkeypatch):
    from comapreduce_amd.mapmaking.destriper import DeviceDestriper
    if tile == 'row_major':
        monkeypatch.setenv('COMAP_DS_TILE', '0')
    case = make_case(**CASE_B)
    L, npix, pix = case['L'], case['npix'], case['pix']
    assert pix.size == 60_000
    gid, G = groups_of(case)
    dd = DeviceDestriper(pix, case['tod'], case['w'], L, npix, map_shape=(64, 64), residuals=True,
                         residual_groups=(case['feed'], case['obs']))
    assert (dd.layout is not None) == (tile == 'tiled')
    res = dd.solve(1e-6, 50)
    assert set(res) == {'x', 'iters', 'maps', 'residuals'}
    assert set(res['residuals']) == {'chi2', 'sum', 'count', 'offset_sum', 'offset_count'}
    r = check_tables(res, pix, case['tod'], case['w'], L, gid, G)
    assert r['chi2'].shape == (G,) and r['offset_sum'].shape == (pix.size // L,)
    counted = int(np.sum((pix >= 0) & (case['w'] > 0)))
    assert int(r['count'].sum()) == counted == int(r['offset_count'].sum())
    # explicit labels give the same tables; the to_host call returns host arrays with the same bits
    res2 = DeviceDestriper(pix, case['tod'], case['w'], L, npix, map_shape=(64, 64), residuals=(gid, G)).solve(
        1e-6, 50, to_host=True)
    for k, v in r.items():
        assert isinstance(res2['residuals'][k], np.ndarray) and np.array_equal(res2['residuals'][k], v), k
    assert np.array_equal(res2['maps']['map'], res['maps']['map'].cpu().numpy(), equal_nan=True)


# ---------------------------------------------------------------- 5. the cut
def noisy_case(params):
    """The case's geometry with a sky, a drift per offset and white noise of sigma = 0.1, five
    times that in the last (observation, feed) group, under weights that claim 1 / sigma^2."""
    case = make_case(**params)
    L, npix, pix = case['L'], case['npix'], case['pix']
    gid, G = groups_of(case)
    rng = np.random.default_rng(21)
    sigma = 0.1
    w = np.where(case['w'] > 0, 1.0 / sigma ** 2, 0.0)
    sky = 2.0 * rng.standard_normal(npix)
    n = pix.size
    scale = np.where(np.repeat(gid, L) == G - 1, 5.0, 1.0)
    tod = sky[pix % npix] + np.repeat(np.cumsum(0.3 * rng.standard_normal(n // L)), L) \
        + scale * sigma * rng.standard_normal(n)
    return case, tod, w, gid, G


@pytest.mark.parametrize('which', ['A', 'B'])
def test_cut_removes_the_noisy_group(which):
    """On the CPU oracle this recipe gives, with residual_cut = 5: first pass 1.55-1.96 (A) and
    1.29-1.32 (B) for the good groups, 14.7 (A) and 21.8 (B) for the noisy one; after the cut the
    survivors are at 0.97-1.42 (A) and 0.98-1.02 (B)."""
    from comapreduce_amd.mapmaking.destriper import DeviceDestriper
    case, tod, w, gid, G = noisy_case(CASE_A if which == 'A' else CASE_B)
    L, npix, pix = case['L'], case['npix'], case['pix']
    shape = None if which == 'A' else (64, 64)
    groups = (case['feed'], case['obs'])
    res = DeviceDestriper(pix, tod, w, L, npix, map_shape=shape, residual_groups=groups, residual_cut=5.0).solve(1e-6, 100)
    r = {k: v.cpu().numpy() for k, v in res['residuals'].items()}
    assert set(r) == {'chi2', 'sum', 'count', 'offset_sum', 'offset_count', 'cut', 'chi2_first'}
    print(which, 'chi2_first', r['chi2_first'], 'chi2', r['chi2'])
    held = np.bincount(gid, minlength=G) > 0
    want_cut = np.zeros(G, bool)
    want_cut[G - 1] = True
    assert r['cut'].dtype == bool and np.array_equal(r['cut'], want_cut)
    assert r['chi2_first'][G - 1] > 5 and np.all(r['chi2_first'][:G - 1] < 5)
    assert np.all(r['chi2_first'][held] > 0)
    # the second solve is the plain solve of the hand-cut problem
    gone = gid == G - 1
    w_cut = np.where(np.repeat(gone, L), 0.0, w)
    keep = (~gone).astype(np.uint8)[None, :]
    plain = DeviceDestriper(pix, tod, w_cut, L, npix, keep=keep, map_shape=shape).solve(1e-6, 100)
    assert set(plain['maps']) == set(res['maps']) >= {'map', 'naive', 'weight', 'hits'}
    for k in plain['maps']:
        assert np.array_equal(res['maps'][k].cpu().numpy(), plain['maps'][k].cpu().numpy(), equal_nan=True), k
    assert np.array_equal(res['x'].cpu().numpy(), plain['x'].cpu().numpy())
    assert r['count'][G - 1] == 0 and r['chi2'][G - 1] == 0.0 and np.all(r['offset_count'][gone] == 0)
    assert np.all(r['chi2'][:G - 1] < 5)
    check_tables(res, pix, tod, w_cut, L, gid, G, keep=keep)
    # a cut nothing reaches: no second solve, the uncut solve's bytes
    loose = DeviceDestriper(pix, tod, w, L, npix, map_shape=shape, residual_groups=groups, residual_cut=1e9).solve(1e-6, 100)
    uncut = DeviceDestriper(pix, tod, w, L, npix, map_shape=shape).solve(1e-6, 100)
    assert not loose['residuals']['cut'].cpu().numpy().any()
    assert np.array_equal(loose['residuals']['chi2'].cpu().numpy(), r['chi2_first'])
    for k in uncut['maps']:
        assert loose['maps'][k].cpu().numpy().tobytes() == uncut['maps'][k].cpu().numpy().tobytes(), k
    assert loose['x'].cpu().numpy().tobytes() == uncut['x'].cpu().numpy().tobytes()


def test_errors_and_nan():
    """Not with the ground template; labels are checked; a non-finite tod of a counted sample makes
    its offset's and its group's sums NaN and nobody else's."""
    from comapreduce_amd.mapmaking.destriper import DeviceDestriper, run_destriper
    case, tod, w, gid, G = noisy_case(CASE_A)
    L, npix, pix = case['L'], case['npix'], case['pix']
    groups = (case['feed'], case['obs'])
    with pytest.raises(NotImplementedError):
        DeviceDestriper(pix, tod, w, L, npix, ground=(case['az'], *groups), residuals=True, residual_groups=groups)
    with pytest.raises(NotImplementedError):
        run_destriper(pix, tod, w, L, np.arange(npix), az=case['az'], feedid=case['feed'], obsids=case['obs'],
                      ground=True, residual_cut=5.0)
    with pytest.raises(ValueError):
        DeviceDestriper(pix, tod, w, L, npix, residuals=True)                       # no groups to label with
    with pytest.raises(ValueError):
        DeviceDestriper(pix, tod, w, L, npix, residuals=(gid, G - 1))               # a label >= n_groups
    t = int(np.nonzero((np.repeat(gid, L) == 0) & (pix >= 0) & (w > 0))[0][3])
    tod = tod.copy()
    tod[t] = np.nan
    rng = np.random.default_rng(4)
    x, m = rng.standard_normal(gid.size), rng.standard_normal(npix)
    rc, got, msg = raw_call(pix, tod[None], w[None], x[:, None], m[:, None], gid, G, L, npix)
    assert rc == 0, msg
    assert np.isnan(got[0][t // L, 0]) and np.isnan(got[2][0, 0])
    assert np.isfinite(np.delete(got[0][:, 0], t // L)).all() and np.isfinite(got[2][1:, 0]).all()
    assert np.array_equal(got[1][:, 0], restate(pix, tod, w, x, m, L)[1])           # still counted


# ---------------------------------------------------------------- 6. the drivers
def test_drivers_return_the_tables():
    from comapreduce_amd.mapmaking.destriper import run_destriper, run_destriper_bands
    case, tod, w, gid, G = noisy_case(CASE_A)
    L, npix, pix = case['L'], case['npix'], case['pix']
    edges = np.arange(npix)
    ids = dict(feedid=case['feed'], obsids=case['obs'])
    assert set(run_destriper(pix, tod, w, L, edges, **ids)) == {'All'}
    first = run_destriper(pix, tod, w, L, edges, residuals=True, **ids)
    assert set(first) == {'All', 'Residuals'} and set(first['Residuals']) == {'obsids', 'feeds', 'chi2', 'count'}
    t = first['Residuals']
    assert t['obsids'].tolist() == [100, 107] and t['feeds'].tolist() == [1, 4, 7]
    assert t['chi2'].shape == t['count'].shape == (2, 3)
    assert t['count'][1, 1] == 0 and t['chi2'][1, 1] == 0.0 and np.sum(t['count'] == 0) == 1
    assert int(t['count'].sum()) == int(np.sum((pix >= 0) & (w > 0)))
    out = run_destriper(pix, tod, w, L, edges, residual_cut=5.0, **ids)
    t = out['Residuals']
    assert set(t) == {'obsids', 'feeds', 'chi2', 'count', 'cut', 'chi2_first'}
    assert t['cut'].shape == (2, 3) and t['cut'].sum() == 1 and t['cut'][1, 2] and t['chi2_first'][1, 2] > 5
    # bands
    tods, ws = np.stack([tod, tod[::-1].copy()]), np.stack([w, w])
    plain = run_destriper_bands(pix, tods, ws, L, edges)
    assert [set(b) for b in plain] == [{'All', 'iters', 'offsets'}] * 2
    bands = run_destriper_bands(pix, tods, ws, L, edges, residuals=True, **ids)
    assert [set(b) for b in bands] == [{'All', 'iters', 'offsets', 'Residuals'}] * 2
    for b in bands:
        assert set(b['Residuals']) == {'obsids', 'feeds', 'chi2', 'count'}
        assert b['Residuals']['chi2'].shape == (2, 3) and b['Residuals']['count'][1, 1] == 0
    assert np.array_equal(bands[0]['Residuals']['count'], first['Residuals']['count'])
    assert not np.array_equal(bands[0]['Residuals']['chi2'], bands[1]['Residuals']['chi2'])
    for k in plain[0]['All']:
        assert np.array_equal(plain[0]['All'][k], bands[0]['All'][k], equal_nan=True), k


def test_main_writes_the_table(tmp_path):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
    import comapdata_case as cc
    from comapreduce_amd.mapmaking.run_destriper import main
    store, names = cc.store()
    m = cc.CASES['car']['map']
    geo = dict(nxpix=m['nxpix'], nypix=m['nypix'], crval=m['crval'], crpix=m['crpix'], ctype=m['ctype'],
               cdelt=m['cdelt'])
    kw = dict(offset_length=50, prefix='t', feeds=cc.FEEDS, use_gain_filter=True, calibration=False, threshold=1e-6,
              niter=50, bands=(0, 1), store=store, **geo)
    for mode, batch in (('batched', True), ('per_band', False)):
        out = main(names[:2], output_dir=str(tmp_path / mode), batch_bands=batch, residuals=True, **kw)
        for b in (0, 1):
            t = out[b]['Residuals']
            z = np.load(str(tmp_path / mode / f't_residuals_band{b}.npz'))
            assert set(z.files) == {'obsids', 'feeds', 'chi2', 'count'}
            assert z['chi2'].shape == (2, len(cc.FEEDS)) and z['obsids'].tolist() == [12, 13]
            for k in z.files:
                assert np.array_equal(z[k], t[k]), (mode, b, k)
            assert z['count'].sum() > 0 and np.all(np.isfinite(z['chi2'])) and np.all(z['chi2'][z['count'] > 0] > 0)
